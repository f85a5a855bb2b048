#!/usr/bin/env python3
"""Per-instance time of the batched dense KKT backend (piqp_amd.BatchDenseKKT, pq_kkt_batch_*) next to ONE single handle of the same shape (piqp_amd.DenseKKT,
pq_kkt_create_dense, with dense_cholesky and with dense_cholesky_exact) and to the oracle's dense backend on one host core.
    python tools/dense_kkt_batch_timing.py > profiles/dense_kkt_batch_timing.txt
batch = 4096 instances, all different, (n, p, m) = (8, 2, 16), (32, 8, 64), (64, 16, 128), (128, 32, 256); data and vectors resident in device memory.
Columns, microseconds:
  factor/inst, solve/inst   hipEvent time of the ONE update_scalings_and_factor launch (reciprocal + assembly + factorisation of every instance) resp. of the one
                            solve launch, divided by the batch (BatchDenseKKT.last_ms)
  single, exact             hipEvent time of the launches of ONE update_scalings_and_factor (stages 0 + 1 of the handle's profile: reciprocal, assembly, panels)
                            resp. ONE solve (stage 2) of a single handle: what a loop over single handles pays per instance on the device alone (each whole call
                            costs more: launches, the status read-back)
  oracle                    orc_kkt_update_scalings_and_factor resp. orc_kkt_solve of one instance on one core
What is NOT timed: the copies of host-mode calls, the status read-back, create / update_data (A' A).
The device measurements alternate in one process, ROUNDS rounds of REPS calls each; every figure is the median over the rounds of the round's median, the spread is
(max - min) / median of the rounds' medians of the batched launch.  Requirement recorded: the batched launch takes less device time than `batch` single-handle calls."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import piqp_amd as hip  # noqa: E402
from oracle import pyorc as orc  # noqa: E402  (the CPU side of the table)

BATCH, ROUNDS, REPS = 4096, 7, 5
SHAPES = ((8, 2, 16), (32, 8, 64), (64, 16, 128), (128, 32, 256))


def qp_batch(n, p, m, batch, seed):
    """P[i] diagonally dominant symmetric, A[i] and G[i] dense, every instance different (cheap to build for 4096 of them)"""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((batch, n, n)), 1)
    P = U + U.transpose(0, 2, 1)
    P[:, np.arange(n), np.arange(n)] = np.abs(P).sum(axis=2) + 1.0
    return P, rng.standard_normal((batch, p, n)), rng.standard_normal((batch, m, n)), rng


def med(f, reps):
    x = []
    for _ in range(reps):
        x.append(f())
    return float(np.median(x))


def single_ms(k, sc, rhs):
    """(device ms of one factor call, device ms of one solve) of a single handle, from its hipEvent brackets"""
    assert k.update_scalings_and_factor(*sc)
    f = k.get_profile(0)[0] + k.get_profile(1)[0]
    k.solve(*rhs)
    return f, k.get_profile(2)[0]


def oracle_us(q, sc, rhs, budget_s=0.2):
    od = orc.Data.dense(**q)
    ko = orc.KKT(od)
    tf, ts, t_all = [], [], 0.0
    while t_all < budget_s or len(tf) < 5:
        t0 = time.perf_counter()
        ok = ko.update_scalings_and_factor(*sc)
        t1 = time.perf_counter()
        ko.solve(*rhs)
        t2 = time.perf_counter()
        assert ok
        tf.append(t1 - t0); ts.append(t2 - t1); t_all += t2 - t0
    return float(np.median(tf)) * 1e6, float(np.median(ts)) * 1e6


def main():
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    print(f"# update_scalings_and_factor and solve of {BATCH} dense KKT instances in one launch each (kkt_solver = dense_cholesky), microseconds PER INSTANCE,")
    print("# next to one single handle (dense_cholesky, dense_cholesky_exact; device time of one call) and one host core")
    print(f"# median over {ROUNDS} alternating rounds of {REPS} calls each; spread = (max - min) / median over the rounds, batched launch")
    print(f"{'n':>4} {'p':>3} {'m':>4} {'what':>7} | {'batch/inst':>10} {'launch':>9} {'spread':>7} | {'single':>8} {'exact':>8} {'oracle':>8} | single / batch, exact / batch, oracle / batch")
    for n, p, m in SHAPES:
        P, A, G, rng = qp_batch(n, p, m, BATCH, n)
        kb = hip.BatchDenseKKT(dev(P), dev(A), dev(G))  # (P symmetric: row-major = column-major)
        delta, x_reg, z_reg = 10.0 ** rng.uniform(-9, -3, BATCH), 10.0 ** rng.uniform(-9, -3, (BATCH, n)), 10.0 ** rng.uniform(-6, 3, (BATCH, m))
        rhs = rng.standard_normal((BATCH, n)), rng.standard_normal((BATCH, p)), rng.standard_normal((BATCH, m))
        dsc, drhs = [dev(a) for a in (delta, x_reg, z_reg)], [dev(a) for a in rhs]
        dout = [torch.empty_like(a) for a in drhs]
        q0 = dict(P=P[0], c=np.zeros(n), A=A[0], b=np.zeros(p), G=G[0], h_l=-np.ones(m), h_u=np.ones(m))
        sc0, rhs0 = (float(delta[0]), x_reg[0], z_reg[0]), tuple(a[0] for a in rhs)
        dsc0 = (sc0[0], dev(sc0[1]), dev(sc0[2]))
        drhs0 = tuple(dev(a) for a in rhs0)
        singles = []
        for ks in (hip.DENSE_CHOLESKY, hip.DENSE_CHOLESKY_EXACT):
            k1 = hip.DenseKKT(hip.Data(**q0), kkt_solver=ks)
            k1.set_profiling(True)
            singles.append(k1)

        def batch_ms():
            assert kb.update_scalings_and_factor(*dsc) == BATCH
            kb.solve(*drhs, out=dout)
            return kb.last_ms()[:2]
        for _ in range(3):
            batch_ms()
            for k1 in singles:
                single_ms(k1, dsc0, drhs0)
        rb, rs = [], [[], []]
        for _ in range(ROUNDS):
            x = [batch_ms() for _ in range(REPS)]
            rb.append(np.median(np.array(x), axis=0))
            for j, k1 in enumerate(singles):
                x = [single_ms(k1, dsc0, drhs0) for _ in range(REPS)]
                rs[j].append(np.median(np.array(x), axis=0))
        rb = np.array(rb) * 1e3
        launch = np.median(rb, axis=0)
        spread = (rb.max(axis=0) - rb.min(axis=0)) / launch
        single = [np.median(np.array(r), axis=0) * 1e3 for r in rs]
        o_us = oracle_us(q0, sc0, rhs0)
        for w, what in enumerate(("factor", "solve")):
            per = launch[w] / BATCH
            verdict = "batch < 4096 x single: yes" if launch[w] * (1 + spread[w]) < BATCH * min(single[0][w], single[1][w]) else "batch < 4096 x single: NO"
            print(f"{n:4d} {p:3d} {m:4d} {what:>7} | {per:10.4f} {launch[w]:9.1f} {100 * spread[w]:6.1f}% | {single[0][w]:8.1f} {single[1][w]:8.1f} {o_us[w]:8.2f} | "
                  f"{single[0][w] / per:8.1f}x {single[1][w] / per:8.1f}x {o_us[w] / per:8.2f}x  {verdict}", flush=True)
        del kb, singles


if __name__ == "__main__":
    main()
