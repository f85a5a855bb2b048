#!/usr/bin/env python3
"""What BatchDenseSolver.update() costs next to the only way to the same state without it, setup() of the same data on the same handle.
    python tools/dense_solver_batch_update_timing.py > profiles/dense_solver_batch_update_timing.txt
batch = 4096 QPs at the four shapes and with the inputs of tools/dense_solver_batch_timing.py; kkt_solver = dense_cholesky; default settings (so an update that
carries a matrix runs the equilibration again, as a setup does); every array is host memory (NumPy), for update() and for setup() alike.  Per shape, medians over
ROUNDS alternating rounds in one process, each round: update(vectors), solve(), setup(the same data), solve(), update(all), setup(the same data), setup(the first
problem).  So every timed update(vectors) is the first call after a setup(); the loop it is meant for, update(vectors) and solve() again and again on one handle, is
timed after the rounds (ROUNDS times) and given on a line of its own.
  vectors  c, b, h_l, h_u, x_l, x_u of the problem moved a little (the bounds widened by 0.25 around a shifted point); the matrices stay
  all      all nine arrays of a second batch drawn with another seed
wall is the time of the Python call; device is what pq_solver_batch_last_update_ms reports (hipEvents around the kernels and copies of the update).  setup() spreads
its work over two streams with host-side waits between them and has no single device interval: it is given as wall time only.  No ratio is fixed in advance."""
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
    print(f"# BatchDenseSolver.update() against setup() of the same data on the same handle, {BATCH} QPs, host arrays, default settings; medians over {ROUNDS} alternating rounds;"
          " ms are per batch, us per QP")
    for n, p, m in SHAPES:
        seed = 1000 * n + 10 * p + m
        q = qp_batch(n, p, m, BATCH, seed)
        rng = np.random.default_rng(seed + 7)
        d = 0.01 * rng.standard_normal((BATCH, n))
        Ad, Gd = np.einsum("bij,bj->bi", q["A"], d), np.einsum("bij,bj->bi", q["G"], d)
        vec = dict(c=q["c"] + 0.1 * rng.standard_normal((BATCH, n)), b=q["b"] + Ad, h_l=q["h_l"] + Gd - 0.25, h_u=q["h_u"] + Gd + 0.25, x_l=q["x_l"] + d - 0.25,
                   x_u=q["x_u"] + d + 0.25)
        q_vec = dict(q, **vec)
        q_all = qp_batch(n, p, m, BATCH, seed + 1)
        s = hip.BatchDenseSolver()
        s.setup(**q)
        s.solve()
        s.update(**vec)  # warm-up of the update's kernels
        rec = {k: [] for k in ("uv", "uv_dev", "uv_solve", "sv", "sv_solve", "ua", "ua_dev", "sa")}
        solved = []
        for _ in range(ROUNDS):
            t, _ = timed(lambda: s.update(**vec))
            rec["uv"].append(t)
            rec["uv_dev"].append(s.last_update_ms()["device_ms"])
            ts, k = timed(s.solve)
            rec["uv_solve"].append(t + ts)
            solved.append(k)
            t, _ = timed(lambda: s.setup(**q_vec))
            rec["sv"].append(t)
            ts, k = timed(s.solve)
            rec["sv_solve"].append(t + ts)
            solved.append(k)
            t, _ = timed(lambda: s.update(**q_all))
            rec["ua"].append(t)
            rec["ua_dev"].append(s.last_update_ms()["device_ms"])
            t, _ = timed(lambda: s.setup(**q_all))
            rec["sa"].append(t)
            s.setup(**q)  # back to the first problem for the next round
        rec["uv_loop"], rec["uv_loop_dev"] = [], []
        for _ in range(ROUNDS):
            s.solve()
            t, _ = timed(lambda: s.update(**vec))
            rec["uv_loop"].append(t)
            rec["uv_loop_dev"].append(s.last_update_ms()["device_ms"])
        med = {k: float(np.median(v)) for k, v in rec.items()}
        us = lambda ms: 1e3 * ms / BATCH
        print(f"n = {n}, p = {p}, m = {m}: solves after update(vectors) and after setup() of the same data ended SOLVED in {min(solved)} .. {max(solved)} of {BATCH}")
        print(f"  update(vectors)          wall {med['uv']:9.2f} ms ({us(med['uv']):8.2f} us)   device {med['uv_dev']:9.2f} ms ({us(med['uv_dev']):8.2f} us)"
              f"   setup() wall {med['sv']:9.2f} ms ({us(med['sv']):8.2f} us)   setup / update = {med['sv'] / med['uv']:.1f}x")
        print(f"  update(vectors) in a loop wall {med['uv_loop']:8.2f} ms ({us(med['uv_loop']):8.2f} us)   device {med['uv_loop_dev']:9.2f} ms ({us(med['uv_loop_dev']):8.2f} us)"
              f"   (after a solve(), not after a setup())")
        print(f"  update(all)              wall {med['ua']:9.2f} ms ({us(med['ua']):8.2f} us)   device {med['ua_dev']:9.2f} ms ({us(med['ua_dev']):8.2f} us)"
              f"   setup() wall {med['sa']:9.2f} ms ({us(med['sa']):8.2f} us)   setup / update = {med['sa'] / med['ua']:.1f}x"
              + ("" if med["ua"] < med["sa"] else "   update(all) is NOT below setup() here"))
        print(f"  update(vectors) + solve  wall {med['uv_solve']:9.2f} ms ({us(med['uv_solve']):8.2f} us)   setup() + solve() wall {med['sv_solve']:9.2f} ms ({us(med['sv_solve']):8.2f} us)"
              f"   ratio {med['sv_solve'] / med['uv_solve']:.2f}x")
        del s
    return 0


if __name__ == "__main__":
    sys.exit(main())
