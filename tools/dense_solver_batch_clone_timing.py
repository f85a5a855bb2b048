#!/usr/bin/env python3
"""What BatchDenseSolver.clone() costs next to the only other way to a second set-up handle, setup() of the same data.
    python tools/dense_solver_batch_clone_timing.py > profiles/dense_solver_batch_clone_timing.txt
batch = 4096 QPs at the four shapes and with the inputs of tools/dense_solver_batch_timing.py; kkt_solver = dense_cholesky; default settings; host arrays (NumPy) for
setup().  Per shape, medians over ROUNDS alternating rounds in one process, each round: clone() of the set-up and solved source, solve() of that clone, solve() of the
source, clone(instances = a fixed permutation of the batch), setup() of the same data on a second handle.  The clones of a round are released before the next one.
  wall     the time of the Python call
  device   what pq_solver_batch_clone_ms reports: the hipEvent time of the gathers of the three layers; wall minus device is allocation (several dozen buffers), the
           upload of the list and the host images
  rate     bytes read plus written by the gathers of the backend's matrix buffers (P, A', G', A'A and the factor store: 2 x 8 x batch x (3 n n + n p + n m)) over the
           device time of the WHOLE clone -- the hundred small gathers ride in that time, so the figure is a lower bound of what the gather kernel moves on the large
           rows -- beside pq_microbench_hbm_copy of the same run
setup() spreads its work over two streams with host-side waits between them and has no single device interval: wall time only.  The setup() column of
tools/dense_solver_batch_update_timing.py, run beside this tool, is the same call on a handle of the parent's code.  No ratio is fixed in advance."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import piqp_amd as hip  # noqa: E402
from dense_solver_batch_timing import BATCH, ROUNDS, SHAPES, qp_batch  # noqa: E402


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    L = hip._lib.load()
    gb = C.c_double(0.0)
    assert L.pq_microbench_hbm_copy(0, 512 << 20, 20, C.byref(gb)) == 0
    print(f"# BatchDenseSolver.clone() against setup() of the same data, {BATCH} QPs, default settings; medians over {ROUNDS} alternating rounds; ms are per batch")
    print(f"# pq_microbench_hbm_copy (512 MiB): {gb.value:.0f} GB/s read + write")
    below = True
    for n, p, m in SHAPES:
        seed = 1000 * n + 10 * p + m
        q = qp_batch(n, p, m, BATCH, seed)
        perm = np.random.default_rng(seed + 3).permutation(BATCH)
        s = hip.BatchDenseSolver()
        s.setup(**q)
        other = hip.BatchDenseSolver()
        other.setup(**q)
        solved = s.solve()
        w = s.clone()  # warm-up of the gather kernels and of the clone's solve
        w.solve()
        del w
        rec = {k: [] for k in ("cw", "cd", "pw", "pd", "setup", "src", "cl")}
        for _ in range(ROUNDS):
            t, c = timed(s.clone)
            rec["cw"].append(t)
            rec["cd"].append(c.clone_ms()["device_ms"])
            t, k = timed(c.solve)
            assert k == solved
            rec["cl"].append(t)
            del c
            t, _ = timed(s.solve)
            rec["src"].append(t)
            t, c = timed(lambda: s.clone(perm))
            rec["pw"].append(t)
            rec["pd"].append(c.clone_ms()["device_ms"])
            del c
            t, _ = timed(lambda: other.setup(**q))
            rec["setup"].append(t)
        med = {k: float(np.median(v)) for k, v in rec.items()}
        spread = (max(rec["src"]) - min(rec["src"])) / med["src"]
        gbytes = 2 * 8 * BATCH * (3 * n * n + n * p + n * m) / 1e9
        below = below and med["cw"] < med["setup"] and med["pw"] < med["setup"]
        print(f"n = {n}, p = {p}, m = {m}: {solved} of {BATCH} solved; the backend's matrix buffers: {gbytes:.3f} GB read + written per clone")
        for name, w_, d_ in (("clone()           ", "cw", "cd"), ("clone(permutation)", "pw", "pd")):
            print(f"  {name} wall {med[w_]:9.2f} ms   device {med[d_]:9.2f} ms   allocation and host {med[w_] - med[d_]:9.2f} ms   rate >= {gbytes / (1e-3 * med[d_]):7.0f} GB/s"
                  f" ({100 * gbytes / (1e-3 * med[d_]) / gb.value:.0f}% of the copy)   setup() wall {med['setup']:9.2f} ms   setup / clone = {med['setup'] / med[w_]:.1f}x"
                  + ("" if med[w_] < med["setup"] else "   the clone is NOT below setup() here"))
        print(f"  solve() of the source wall {med['src']:9.2f} ms (spread {100 * spread:.1f}% over its rounds)   solve() of the whole clone wall {med['cl']:9.2f} ms"
              f"   clone / source = {med['cl'] / med['src']:.3f}   {'within' if abs(med['cl'] - med['src']) <= max(rec['src']) - min(rec['src']) else 'OUTSIDE'} the source's spread")
        del s, other
    print(f"# a clone, whole or permuted, below setup() at every shape: {'yes' if below else 'NO'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
