"""Wall times of host-fed vs device-fed DenseSolver.setup / update(P, G) at the flagship size, of the batched solver's update(b) -> solve -> result(x)
round trip at 8192 MPC QPs, and the transpose kernel's rate next to the copy micro-benchmark (profiles/device_data_timing.txt).

    python tools/device_data_timing.py [--out FILE] [--parent-lib PATH/libpiqp_amd.so] [--reps N]

Every timed call ends in a drained stream (the library drains its stream at the end of setup / update / result); medians of alternating repetitions.
--parent-lib: a build of the commit before the device-data entry points; its host path is timed through its raw C-ABI in the same process, alternating
with this tree's, so that "host path of the parent" is a measurement and not an assumption."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import piqp_amd  # noqa: E402
from qp_gen import dense_strongly_convex_qp, mpc_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_data_timing.txt"))
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--device", type=int, default=0)
args = ap.parse_args()
OUT = args.out
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def write_record():
    """once, at the end: a run that dies half-way leaves the previous record alone"""
    tmp = OUT + ".tmp"
    with open(tmp, "w") as f:
        f.write("\n".join(lines) + "\n")
    os.replace(tmp, OUT)


def med(v):
    return statistics.median(v), min(v), max(v)


def fmt(name, v):
    m, lo, hi = med(v)
    return f"{name:<58s} median {m * 1e3:9.3f} ms   (min {lo * 1e3:9.3f}, max {hi * 1e3:9.3f}, {len(v)} runs)"


REPS = args.reps
n = m = 4096
L = piqp_amd._lib.load()
DEV = args.device
torch.cuda.set_device(DEV)
say(f"device-data timing on {torch.cuda.get_device_name(DEV)} (device {DEV}), n = m = {n}, p = 0 (the bench.py flagship shape), dense_cholesky; torch {torch.__version__}")
say("taken with tools/device_data_timing.py" + (" --parent-lib <build of the parent commit>" if args.parent_lib else ""))
q = dense_strongly_convex_qp(n, 0, m, seed=43, double_sided=True, exact_shift=False)
q = {k: v for k, v in q.items() if v is not None}
row = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in q.items()}
col = dict(row)
for k in ("P", "G"):
    col[k] = torch.from_numpy(np.ascontiguousarray(q[k].T)).cuda().t()
qF = dict(q)
for k in ("P", "G"):
    qF[k] = np.asfortranarray(q[k])  # what the host entry takes without a conversion in the binding
torch.cuda.synchronize()

# ---- the parent commit's library, host path, through its raw C-ABI (the binding of this tree names symbols it does not have)
vp = C.c_void_p
PL = C.CDLL(args.parent_lib) if args.parent_lib else None
if PL is not None:
    PL.pq_solver_create.argtypes = [C.POINTER(vp), C.c_int]
    PL.pq_solver_destroy.argtypes = [vp]; PL.pq_solver_destroy.restype = None
    PL.pq_solver_setup_dense.argtypes = [vp, C.c_int, C.c_int, C.c_int] + [vp] * 9
    PL.pq_solver_update_dense.argtypes = [vp] + [vp] * 9
NAMES = ("P", "c", "A", "b", "G", "h_l", "h_u", "x_l", "x_u")


def raw_ptrs(d):
    return [d[k].ctypes.data if k in d else None for k in NAMES]


def parent_setup():
    h = vp()
    assert PL.pq_solver_create(C.byref(h), DEV) == 0
    t = time.perf_counter()
    assert PL.pq_solver_setup_dense(h, n, 0, m, *raw_ptrs(qF)) == 1
    return h, time.perf_counter() - t


def parent_update(h):
    t = time.perf_counter()
    assert PL.pq_solver_update_dense(h, *raw_ptrs(dict(P=qF["P"], G=qF["G"]))) == 1
    return time.perf_counter() - t


def new_setup(args):
    s = piqp_amd.DenseSolver(device=DEV)
    t = time.perf_counter()
    assert s.setup(**args)
    return s, time.perf_counter() - t


def new_update(s, args):
    t = time.perf_counter()
    assert s.update(P=args["P"], G=args["G"])
    return time.perf_counter() - t


# warm-up of every path (code objects, pinned staging)
s, _ = new_setup(qF); new_update(s, qF); del s
s, _ = new_setup(row); new_update(s, row); new_update(s, col); del s
if PL is not None:
    h, _ = parent_setup(); parent_update(h); PL.pq_solver_destroy(h)

T = {k: [] for k in ("ps", "pu", "hs", "hu", "rs", "ru", "cs", "cu")}
for _ in range(REPS):
    if PL is not None:
        h, t = parent_setup(); T["ps"].append(t); T["pu"].append(parent_update(h)); PL.pq_solver_destroy(h)
    s, t = new_setup(qF); T["hs"].append(t); T["hu"].append(new_update(s, qF)); del s
    s, t = new_setup(row); T["rs"].append(t); T["ru"].append(new_update(s, row)); ing = s.last_ingest(); del s
    s, t = new_setup(col); T["cs"].append(t); T["cu"].append(new_update(s, col)); del s
say()
say("setup(P, c, G, h_l, h_u, x_l, x_u): wall time of the call (returns with the library's stream drained)")
if PL is not None:
    say(fmt("  parent commit, host arrays (column-major numpy)", T["ps"]))
say(fmt("  this tree, host arrays (column-major numpy)", T["hs"]))
say(fmt("  this tree, CUDA tensors, row-major (contiguous)", T["rs"]))
say(fmt("  this tree, CUDA tensors, column-major (transposed view)", T["cs"]))
say("update(P, G): wall time of the call")
if PL is not None:
    say(fmt("  parent commit, host arrays", T["pu"]))
say(fmt("  this tree, host arrays", T["hu"]))
say(fmt("  this tree, CUDA tensors, row-major", T["ru"]))
say(fmt("  this tree, CUDA tensors, column-major", T["cu"]))
say(f"  pq_solver_last_ingest after the device-fed update: link bytes {ing[0]}, device bytes {ing[1]}")

# ---- transpose kernel vs the copy micro-benchmark, same run
say()
gb = C.c_double()
assert L.pq_microbench_hbm_copy(DEV, 512 << 20, 20, C.byref(gb)) == 0
copy_rate = gb.value
say(f"pq_microbench_hbm_copy (512 MiB, best shape): {copy_rate:8.0f} GB/s read + write")
for r, c in ((4096, 4096), (8192, 8192), (4096, 1024), (4097, 4099)):
    assert L.pq_microbench_transpose(DEV, r, c, 50, C.byref(gb)) == 0
    say(f"pq_microbench_transpose {r:5d} x {c:5d} fp64 ({r * c * 8 / 2**20:6.1f} MiB): {gb.value:8.0f} GB/s read + write  = {gb.value / copy_rate:5.2f} of the copy rate")

# ---- batch round trip, 8192 MPC QPs (C4)
say()
B = 8192
mb = mpc_batch(B, seed=1000)
bs = piqp_amd.BatchSparseSolver(device=DEV)
assert bs.setup(mb["P_pattern"], mb["P_values"], mb["c"], mb["A_pattern"], mb["A_values"], mb["b"], x_l=mb["x_l"], x_u=mb["x_u"])
assert bs.solve() == B
rng = np.random.default_rng(1)
states = [mb["b"].copy() for _ in range(4)]
for b in states:
    b[:, :2] = rng.uniform(-0.8, 0.8, (B, 2))
states_gpu = [torch.from_numpy(b).cuda() for b in states]
torch.cuda.synchronize()


def trip(host, b):
    t0 = time.perf_counter()
    bs.update(b=b)
    t1 = time.perf_counter()
    bs.solve()
    t2 = time.perf_counter()
    x = bs.result("x") if host else bs.result("x", device=True)
    if not host:
        torch.cuda.synchronize()
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2, t3 - t0, x


for k in range(2):
    trip(True, states[k]); trip(False, states_gpu[k])
R = {True: [], False: []}
same = True
for rep in range(REPS):
    k = rep % len(states)
    a = trip(True, states[k]); R[True].append(a[:4])
    d = trip(False, states_gpu[k]); R[False].append(d[:4])
    same = same and np.array_equal(a[4].view(np.uint64), d[4].cpu().numpy().view(np.uint64))
say(f"batch of {B} MPC QPs (n = {mb['n']}, p = {mb['p']}), sparse_multistage: update(b) -> solve() -> result('x'); x bitwise equal between the two paths: {same}")
for host, nm in ((True, "host arrays (numpy in, numpy out)"), (False, "CUDA tensors (in place in, torch tensor out)")):
    v = R[host]
    say(f"  {nm}")
    for i, part in enumerate(("update(b)", "solve()", "result('x')", "round trip")):
        say(fmt(f"    {part}", [r[i] for r in v]))
write_record()
