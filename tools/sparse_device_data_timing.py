"""Wall times of host-fed vs device-fed SparseSolver.update(P, A, G) -- and setup -- on the C3 recipe of bench.py (n = 50k) and on the Maros-Meszaros fixture
CONT-201, next to the host-fed update of the parent commit (profiles/sparse_device_data_timing.txt).

    python tools/sparse_device_data_timing.py [--out FILE] [--parent-lib PATH/libpiqp_amd.so] [--reps N]

One process, one GPU.  Every timed call goes through the raw C-ABI with argument arrays prepared beforehand -- the parent's library has no binding in this tree, and
the binding's own work on a host-fed call (scipy's sorted-CSC conversion of three matrices, about half a millisecond at these sizes) is the same in both trees and
is not what is compared.  Every timed call ends in a drained stream (the library drains its streams at the end of setup / update); medians of alternating repetitions
after a warm-up of every path.  --parent-lib: a build of the commit before the sparse device-data entry points; its host path is timed through its raw C-ABI in
the same process, alternating with this tree's, so that "the host-fed update is no slower than the parent's" is a measurement.  The record ends with that
comparison: this tree's host-fed median against the parent's median and the spread (max - min) of the parent's own runs."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import piqp_amd  # noqa: E402
from qp_gen import c3_problem  # noqa: E402
from qp_io import load_qp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_device_data_timing.txt"))
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--device", type=int, default=0)
args = ap.parse_args()
assert args.reps >= 3
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def fmt(name, v):
    return f"{name:<52s} median {statistics.median(v) * 1e3:9.3f} ms   (min {min(v) * 1e3:9.3f}, max {max(v) * 1e3:9.3f}, {len(v)} runs)"


DEV = args.device
torch.cuda.set_device(DEV)
vp = C.c_void_p
PL = C.CDLL(args.parent_lib) if args.parent_lib else None
if PL is not None:
    PL.pq_solver_create.argtypes = [C.POINTER(vp), C.c_int]
    PL.pq_solver_destroy.argtypes = [vp]; PL.pq_solver_destroy.restype = None
    PL.pq_solver_settings.argtypes = [vp]; PL.pq_solver_settings.restype = C.POINTER(piqp_amd._lib.Settings)
    PL.pq_solver_setup_sparse.argtypes = [vp, C.c_int, C.c_int, C.c_int] + [vp] * 15
    PL.pq_solver_update_sparse.argtypes = [vp] + [vp] * 15


def csc(M):
    if M is None:
        return [None, None, None]
    M = sp.csc_matrix(M)
    M.sort_indices()
    return [np.ascontiguousarray(M.indptr, dtype=np.int32), np.ascontiguousarray(M.indices, dtype=np.int32), np.ascontiguousarray(M.data, dtype=np.float64)]


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def run_case(title, q, kkt_solver):
    P, c, A, b, G, h_l, h_u, x_l, x_u = q
    n, p, m = P.shape[0], (0 if A is None else A.shape[0]), (0 if G is None else G.shape[0])
    mats = {k: v for k, v in (("P", P), ("A", A), ("G", G)) if v is not None}
    for k in mats:
        mats[k] = sp.csc_matrix(mats[k]); mats[k].sort_indices()
    vecs = dict(c=c, b=b, h_l=h_l, h_u=h_u, x_l=x_l, x_u=x_u)
    host = dict(mats); host.update(vecs)
    dev = {k: (v, cuda(v.data)) for k, v in mats.items()}
    dev.update({k: cuda(v) for k, v in vecs.items()})
    upd_host = dict(mats)
    upd_dev = {k: cuda(v.data) for k, v in mats.items()}
    raw = csc(P) + [c] + csc(A) + [b] + csc(G) + [h_l, h_u, x_l, x_u]
    raw = [None if a is None else np.ascontiguousarray(a) for a in raw]
    ptrs = [None if a is None else a.ctypes.data for a in raw]
    upd_ptrs = [ptrs[i] if i in (0, 1, 2, 4, 5, 6, 8, 9, 10) else None for i in range(15)]
    torch.cuda.synchronize()
    say()
    say(f"{title}: n = {n}, p = {p}, m = {m}, nnz upper(P) / A / G = {sp.triu(mats['P']).nnz} / {A.nnz if A is not None else 0} / {G.nnz if G is not None else 0}, kkt_solver = {kkt_solver}")

    L = piqp_amd._lib.load()
    dptr = lambda k: None if dev.get(k) is None else (dev[k][1] if isinstance(dev[k], tuple) else dev[k]).data_ptr()
    dev_ptrs = [ptrs[0], ptrs[1], dptr("P"), dptr("c"), ptrs[4], ptrs[5], dptr("A"), dptr("b"), ptrs[8], ptrs[9], dptr("G"), dptr("h_l"), dptr("h_u"), dptr("x_l"), dptr("x_u")]
    dev_upd_ptrs = [dev_ptrs[i] if i in (2, 6, 10) else None for i in range(15)]  # values only: the index arrays are not passed again

    def new_solver(a):
        s = piqp_amd.SparseSolver(device=DEV)
        s.settings.kkt_solver = kkt_solver
        t = time.perf_counter()
        if a is host:
            assert L.pq_solver_setup_sparse(s.h, n, p, m, *ptrs) == 1
        else:
            assert L.pq_solver_setup_sparse_mem(s.h, n, p, m, *dev_ptrs, piqp_amd.MEM_DEVICE) == 1
        return s, time.perf_counter() - t

    def new_update(s, a):
        t = time.perf_counter()
        if a is upd_host:
            assert L.pq_solver_update_sparse(s.h, *upd_ptrs) == 1
        else:
            assert L.pq_solver_update_sparse_mem(s.h, *dev_upd_ptrs, piqp_amd.MEM_DEVICE) == 1
        return time.perf_counter() - t

    def parent_solver():
        h = vp()
        assert PL.pq_solver_create(C.byref(h), DEV) == 0
        PL.pq_solver_settings(h).contents.kkt_solver = kkt_solver
        t = time.perf_counter()
        assert PL.pq_solver_setup_sparse(h, n, p, m, *ptrs) == 1
        return h, time.perf_counter() - t

    def parent_update(h):
        t = time.perf_counter()
        assert PL.pq_solver_update_sparse(h, *upd_ptrs) == 1
        return time.perf_counter() - t

    # one solver per path, set up once (the symbolic analysis dominates a setup and is the same in every path); warm-up, then alternating updates
    T = {k: [] for k in ("ps", "hs", "ds", "pu", "hu", "du")}
    sh, t = new_solver(host); T["hs"].append(t)
    sd, t = new_solver(dev); T["ds"].append(t)
    setup_ing = sd.last_ingest()
    ph = None
    if PL is not None:
        ph, t = parent_solver(); T["ps"].append(t)
    for _ in range(2):
        new_update(sh, upd_host); new_update(sd, upd_dev)
        if ph is not None:
            parent_update(ph)
    for _ in range(args.reps):
        if ph is not None:
            T["pu"].append(parent_update(ph))
        T["hu"].append(new_update(sh, upd_host))
        T["du"].append(new_update(sd, upd_dev))
    ing = sd.last_ingest()
    st_h, st_d = sh.solve(), sd.solve()
    rh, rd = sh.result(), sd.result()
    same = st_h == st_d and sh.info.iter == sd.info.iter and all(np.array_equal(rh[k].view(np.uint64), rd[k].view(np.uint64)) for k in rh)
    say("  setup: wall time of the call, one run each (symbolic analysis included)")
    if ph is not None:
        say(f"    parent commit, host arrays                        {T['ps'][0] * 1e3:9.3f} ms")
    say(f"    this tree, host arrays                            {T['hs'][0] * 1e3:9.3f} ms")
    say(f"    this tree, values and vectors in GPU memory       {T['ds'][0] * 1e3:9.3f} ms   (pq_solver_last_ingest: link bytes {setup_ing[0]}, device bytes {setup_ing[1]})")
    say("  update(P, A, G): wall time of the call")
    if ph is not None:
        say(fmt("    parent commit, host arrays", T["pu"]))
    say(fmt("    this tree, host arrays", T["hu"]))
    say(fmt("    this tree, CUDA tensors (values only)", T["du"]))
    say(f"    pq_solver_last_ingest after the device-fed update: link bytes {ing[0]}, device bytes {ing[1]}")
    say(f"    solve after the updates: status {st_h} / {st_d}, {sh.info.iter} / {sd.info.iter} iterations, all ten result vectors bitwise equal between the two paths: {same}")
    if ph is not None:
        mp, mh = statistics.median(T["pu"]), statistics.median(T["hu"])
        spread = max(T["pu"]) - min(T["pu"])
        verdict = "within" if mh - mp <= spread else "OUTSIDE"
        say(f"    host-fed update, this tree - parent: {(mh - mp) * 1e3:+.3f} ms; spread of the parent's own runs {spread * 1e3:.3f} ms: {verdict} the spread")
        PL.pq_solver_destroy(ph)
    del sh, sd


say(f"sparse device-data timing on {torch.cuda.get_device_name(DEV)} (device {DEV}); torch {torch.__version__}")
say("taken with tools/sparse_device_data_timing.py" + (" --parent-lib <build of the parent commit>" if args.parent_lib else ""))
run_case("C3 (the bench.py recipe: qp_gen.c3_problem(seed=44))", c3_problem(seed=44), piqp_amd.SPARSE_LDLT)
q = load_qp("mm_CONT-201")
run_case("Maros-Meszaros CONT-201 (tests/golden/mm_CONT-201.npz)", tuple(q[k] for k in ("P", "c", "A", "b", "G", "h_l", "h_u", "x_l", "x_u")), piqp_amd.SPARSE_LDLT)
tmp = args.out + ".tmp"
with open(tmp, "w") as f:
    f.write("\n".join(lines) + "\n")
os.replace(tmp, args.out)
