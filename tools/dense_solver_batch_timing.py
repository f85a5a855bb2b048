#!/usr/bin/env python3
"""Wall and device time of the batched DenseSolver (piqp_amd.BatchDenseSolver, pq_solver_batch_*) next to the two ways to the same results without it.
    python tools/dense_solver_batch_timing.py > profiles/dense_solver_batch_timing.txt
batch = 4096 feasible QPs, all different, (n, p, m) = (8, 2, 16), (32, 8, 64), (64, 16, 128), (128, 32, 256); every row of G two-sided, every variable boxed on both
sides around a planted point; kkt_solver = dense_cholesky; default settings.  Per shape, medians over ROUNDS alternating rounds in one process:
  batch    solve() of the handle (data resident from setup): wall time and device time summed over its launches (hipEvents), per QP; rounds and launches; the share of
           the factor launches (k_ksb_factor) and the solve launches (k_ksb_solve) in the device time -- the rest is the advance kernel and the final unscaling
  single   a loop over SINGLES piqp_amd.DenseSolver handles (kkt_solver = dense_cholesky_exact, the parent's path to these numbers): wall time of solve() per QP
  oracle   orc.Solver (oracle/, one core) on ORACLES of the instances: wall time of solve() per QP
The one condition: at every shape the batch's wall time per QP is below the oracle's.  The script ends with a line that says whether it held."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import piqp_amd as hip  # noqa: E402
from oracle import pyorc as orc  # noqa: E402

BATCH, ROUNDS, SINGLES, ORACLES = 4096, 7, 16, 16
SHAPES = ((8, 2, 16), (32, 8, 64), (64, 16, 128), (128, 32, 256))


def qp_batch(n, p, m, batch, seed):
    rng = np.random.default_rng(seed)
    k = min(n, 48)
    F = rng.standard_normal((batch, n, k))
    P = F @ F.transpose(0, 2, 1) / k
    P[:, np.arange(n), np.arange(n)] += rng.uniform(0.5, 1.5, (batch, n))
    P = np.triu(P) + np.triu(P, 1).transpose(0, 2, 1)
    A, G, x0 = rng.standard_normal((batch, p, n)), rng.standard_normal((batch, m, n)), rng.standard_normal((batch, n))
    g = np.einsum("bij,bj->bi", G, x0)
    return dict(P=P, c=rng.standard_normal((batch, n)), A=A, b=np.einsum("bij,bj->bi", A, x0), G=G, h_l=g - rng.uniform(0.1, 1.0, (batch, m)),
                h_u=g + rng.uniform(0.1, 1.0, (batch, m)), x_l=x0 - rng.uniform(0.1, 1.0, (batch, n)), x_u=x0 + rng.uniform(0.1, 1.0, (batch, n)))


def main():
    print(f"# the batched DenseSolver, {BATCH} QPs per handle, kkt_solver = dense_cholesky, default settings; medians over {ROUNDS} alternating rounds; us are per QP")
    held = True
    for n, p, m in SHAPES:
        q = qp_batch(n, p, m, BATCH, 1000 * n + 10 * p + m)
        one = lambda i: {k: v[i] for k, v in q.items()}
        s = hip.BatchDenseSolver()
        s.setup(**q)
        singles = []
        for i in range(SINGLES):
            d = hip.DenseSolver()
            d.settings.kkt_solver = hip.DENSE_CHOLESKY_EXACT
            d.setup(**one(i))
            singles.append(d)
        oracles = []
        for i in range(ORACLES):
            o = orc.Solver()
            o.setup(**one(i))
            oracles.append(o)
        solved = s.solve()  # warm-up of everything
        singles[0].solve()
        rec = dict(wall=[], dev=[], fshare=[], sshare=[], single=[], oracle=[])
        for _ in range(ROUNDS):
            s.solve()
            ms = s.last_ms()
            rec["wall"].append(1e3 * ms["wall_ms"] / BATCH)
            rec["dev"].append(1e3 * ms["device_ms"] / BATCH)
            rec["fshare"].append(ms["factor_ms"] / ms["device_ms"])
            rec["sshare"].append(ms["solve_ms"] / ms["device_ms"])
            t0 = time.perf_counter()
            for d in singles:
                d.solve()
            rec["single"].append(1e6 * (time.perf_counter() - t0) / SINGLES)
            t0 = time.perf_counter()
            for o in oracles:
                o.solve()
            rec["oracle"].append(1e6 * (time.perf_counter() - t0) / ORACLES)
        med = {k: float(np.median(v)) for k, v in rec.items()}
        spread = (max(rec["wall"]) - min(rec["wall"])) / med["wall"]
        it = s.iterations()
        ok = med["wall"] < med["oracle"]
        held = held and ok
        print(f"n = {n}, p = {p}, m = {m}: {solved} of {BATCH} solved, iterations {it.min()} .. {it.max()} (mean {it.mean():.1f})")
        print(f"  batch    wall {med['wall']:9.2f} us (spread {100 * spread:.1f}%)   device {med['dev']:9.2f} us   rounds {ms['rounds']}, launches {ms['launches']}"
              f"   of the device time: factor launches {100 * med['fshare']:.0f}%, solve launches {100 * med['sshare']:.0f}%,"
              f" advance and unscaling {100 * (1 - med['fshare'] - med['sshare']):.0f}%   wall / device = {med['wall'] / med['dev']:.2f}")
        print(f"  single   wall {med['single']:9.2f} us over {SINGLES} DenseSolver handles (kkt_solver 19)   single / batch = {med['single'] / med['wall']:.0f}x")
        print(f"  oracle   wall {med['oracle']:9.2f} us over {ORACLES} orc.Solver on one core                 oracle / batch = {med['oracle'] / med['wall']:.1f}x   condition {'holds' if ok else 'FAILS'}")
        del singles, oracles, s
    print(f"# condition (batch wall per QP below the one-core oracle's at every shape): {'holds' if held else 'FAILS'}")
    return 0 if held else 1


if __name__ == "__main__":
    sys.exit(main())
