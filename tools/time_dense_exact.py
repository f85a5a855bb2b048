"""Times the reference-order dense backend (kkt_solver = DENSE_CHOLESKY_EXACT) next to the default dense_cholesky backend and the CPU oracle on one host core:
one update_scalings_and_factor and one solve, n in {64, 256, 512, 1000}, m = n, p = 0.  Device figures are hipEvent brackets on the handle's stream (the
backends' own stage profiler: every kernel of the call, WITHOUT the 4-byte read-back of the factorisation status and the host's wait for it), median of 20 calls
after 5 warm-up calls; the oracle is timed with perf_counter around the whole call, median of 20 after 5.
Usage: python tools/time_dense_exact.py [out.txt]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import piqp_amd as hip  # noqa: E402
from oracle import pyorc as orc  # noqa: E402


def qp(n, m, seed):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((n, 48))
    P = F @ F.T / 48 + np.eye(n)
    return dict(P=np.triu(P) + np.triu(P, 1).T, c=rng.standard_normal(n), G=rng.standard_normal((m, n)), h_l=-np.ones(m), h_u=np.ones(m)), rng


def device(kind, q, x_reg, z_reg, rhs):
    k = hip.DenseKKT(hip.Data(**q), kkt_solver=kind)
    k.set_profiling(True)
    fac, sol = [], []
    for it in range(25):
        assert k.update_scalings_and_factor(1e-6, x_reg, z_reg)
        k.solve(*rhs)
        a, f, s = (k.get_profile(st)[0] for st in (0, 1, 2))
        if it >= 5:
            fac.append(a + f); sol.append(s)
    return statistics.median(fac), statistics.median(sol)


def oracle(q, x_reg, z_reg, rhs):
    orc.lib().orc_set_num_threads(1)
    k = orc.KKT(orc.Data.dense(**q))
    fac, sol = [], []
    for it in range(25):
        t0 = time.perf_counter(); assert k.update_scalings_and_factor(1e-6, x_reg, z_reg); t1 = time.perf_counter()
        k.solve(*rhs); t2 = time.perf_counter()
        if it >= 5:
            fac.append(1e3 * (t1 - t0)); sol.append(1e3 * (t2 - t1))
    return statistics.median(fac), statistics.median(sol)


def main():
    lines = ["# one update_scalings_and_factor / one solve, milliseconds, m = n, p = 0; device: hipEvent brackets around all kernels of the call (not the status read-back and the host's wait for it), median of 20 after 5 warm-up calls; oracle: wall time of the call on one host core",
             f"{'n':>5} {'exact factor':>13} {'exact solve':>12} {'default factor':>15} {'default solve':>14} {'oracle factor':>14} {'oracle solve':>13}"]
    for n in (64, 256, 512, 1000):
        q, rng = qp(n, n, n)
        x_reg, z_reg = np.full(n, 1e-6), rng.uniform(0.1, 10.0, n)
        rhs = (rng.standard_normal(n), np.zeros(0), rng.standard_normal(n))
        e, d, o = device(hip.DENSE_CHOLESKY_EXACT, q, x_reg, z_reg, rhs), device(hip.DENSE_CHOLESKY, q, x_reg, z_reg, rhs), oracle(q, x_reg, z_reg, rhs)
        lines.append(f"{n:>5} {e[0]:>13.4f} {e[1]:>12.4f} {d[0]:>15.4f} {d[1]:>14.4f} {o[0]:>14.4f} {o[1]:>13.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text)


if __name__ == "__main__":
    main()
