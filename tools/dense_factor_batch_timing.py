#!/usr/bin/env python3
"""Per-matrix time of the batched dense factor objects (piqp_amd.BatchLLT / piqp_amd.BatchLDLTNoPivot, pq_dense_factor_batch_*) next to one single object
(piqp_amd.LLT / piqp_amd.LDLTNoPivot, pq_dense_factor_*) and to the oracle's restatement of the same classes on one host core.
    python tools/dense_factor_batch_timing.py > profiles/dense_factor_batch_timing.txt
batch = 4096 matrices of order n = 8, 32, 64, 128, all different, resident in device memory.  Columns, microseconds:
  batch/matrix   hipEvent time of the one factorisation launch divided by the batch
  single         hipEvent time of the factorisation launches of ONE pq_dense_factor_compute of the same order (what a loop over single objects pays per matrix
                 on the device alone; its whole compute() call costs more)
  oracle         orc_llt_compute / orc_ldlt_no_pivot_compute on one core
The two device measurements alternate in one process, ROUNDS rounds of REPS computes each; every figure is the median over the rounds of the round's median."""
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


def spd_batch(n, batch, seed):
    """diagonally dominant symmetric matrices, every one different (cheap to build for 4096 of them)"""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((batch, n, n)), 1)
    S = U + U.transpose(0, 2, 1)
    S[:, np.arange(n), np.arange(n)] = np.abs(S).sum(axis=2) + 1.0
    return S


def oracle_us(S, ldlt, budget_s=0.2):
    n = S.shape[0]
    L = orc.lib()
    w = np.zeros(n)
    ts, t_all = [], 0.0
    while t_all < budget_s or len(ts) < 5:
        a = np.asfortranarray(S.copy())
        t0 = time.perf_counter()
        ret = L.orc_ldlt_no_pivot_compute(a.ctypes.data_as(orc._dp), n, n, w.ctypes.data_as(orc._dp)) if ldlt else L.orc_llt_compute(a.ctypes.data_as(orc._dp), n, n)
        dt = time.perf_counter() - t0
        assert ret == -1
        ts.append(dt); t_all += dt
    return float(np.median(ts)) * 1e6


def main():
    print(f"# compute() of {BATCH} dense positive definite matrices in one launch, microseconds PER MATRIX, next to one single object and one host core")
    print(f"# median over {ROUNDS} alternating rounds of {REPS} computes each")
    print(f"{'n':>4} {'kind':>12} | {'batch/matrix':>12} {'batch launch':>12} | {'single':>8} {'oracle':>8} | single / batch, oracle / batch")
    for n in (8, 32, 64, 128):
        S = spd_batch(n, BATCH, n)
        t = torch.from_numpy(S).cuda()  # symmetric: row-major = column-major
        t1 = torch.from_numpy(S[0].copy()).cuda()
        for name, bcls, scls, ldlt in (("LLT", hip.BatchLLT, hip.LLT, False), ("LDLTNoPivot", hip.BatchLDLTNoPivot, hip.LDLTNoPivot, True)):
            fb, fs = bcls(BATCH, n), scls(n)
            for _ in range(3):
                fb.compute_colmajor(t); fs.compute_colmajor(t1)
            assert fb.n_success == BATCH and fs.info() == 0
            rb, rs = [], []
            for _ in range(ROUNDS):
                x = []
                for _ in range(REPS):
                    fb.compute_colmajor(t); x.append(fb.last_ms()[0])
                rb.append(np.median(x))
                x = []
                for _ in range(REPS):
                    fs.compute_colmajor(t1); x.append(fs.last_ms()[0])
                rs.append(np.median(x))
            launch_us, single_us = float(np.median(rb)) * 1e3, float(np.median(rs)) * 1e3
            per = launch_us / BATCH
            o_us = oracle_us(S[0], ldlt)
            print(f"{n:4d} {name:>12} | {per:12.4f} {launch_us:12.1f} | {single_us:8.1f} {o_us:8.2f} | {single_us / per:8.1f}x {o_us / per:8.2f}x", flush=True)
            del fb, fs


if __name__ == "__main__":
    main()
