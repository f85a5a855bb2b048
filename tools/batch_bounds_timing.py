#!/usr/bin/env python3
"""What the per-instance finite-bound sets of the batched sparse solver cost (piqp_amd.BatchSparseSolver(bounds=...), pq_batch_set_bound_sets).

Two inputs: C4 (qp_gen.mpc_batch(8192), the default sparse_multistage backend) and the sparse benchmark recipe at dim 64 with kkt_solver = sparse_ldlt (4096
perturbed copies, as tools/batch_ldlt_timing.py stacks them).  Three handles per input, timed in one process in 7 alternating rounds, the figure being the median of
pq_batch_last_kernel_ms (the hipEvent time of the solve kernel):
    (a) a handle with shared sets            (b) a handle with sets per instance on the same data            (c) sets per instance, mixed kinds
For (c) every bound that is finite in the input is kept or switched off per instance and per row / variable (kinds 0 .. 3: both, lower, upper, neither, 1/4 each),
which keeps every instance feasible.  Also the wall time of update(h_l, h_u, x_l, x_u) fed from device tensors in (a) and (b), median of 7.
The one condition: (a) not slower than the parent commit by more than the parent's own spread over its rounds.  --shared-only times (a) alone and uses nothing
the parent commit lacks, so the same file runs on the parent's tree; --parent FILE reads such an output and states the condition.  (b) / (a), (c) / (a) and the
update ratios are recorded, not gated.
   python tools/batch_bounds_timing.py --shared-only          (on the parent's tree, before and after)
   python tools/batch_bounds_timing.py --parent parent.txt    (--shared-only --parent: (a) alone, as the parent's process runs it)
profiles/batch_bounds_timing.txt holds the outputs in the order they ran."""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

ROUNDS = 7
BOUNDS = ("h_l", "h_u", "x_l", "x_u")


def inputs():
    import piqp_amd as hip
    from batch_ldlt_timing import stacked
    from dense_sparse_solver_benchmark import sparse_variant
    from qp_gen import dense_strongly_convex_qp, mpc_batch
    mb = mpc_batch(8192)
    c4 = dict(P=mb["P_pattern"], Pv=mb["P_values"], c=mb["c"], A=mb["A_pattern"], Av=mb["A_values"], b=mb["b"], G=None, Gv=None, h_l=None, h_u=None, x_l=mb["x_l"], x_u=mb["x_u"])
    dim = 64
    sv = stacked(sparse_variant(dense_strongly_convex_qp(dim, dim // 2, dim // 2, seed=dim), 0.1, dim), 4096, seed=dim)
    return [("C4 (mpc_batch(8192), sparse_multistage)", c4, hip.SPARSE_MULTISTAGE), ("sparse recipe dim 64, 4096 QPs, sparse_ldlt", sv, hip.SPARSE_LDLT)]


def mixed(st, seed):
    """st with every finite bound kept or switched off per instance"""
    rng = np.random.default_rng(seed)
    out = dict(st)
    for lo, hi in (("h_l", "h_u"), ("x_l", "x_u")):
        if st[lo] is None:
            continue
        kind = rng.integers(0, 4, st[lo].shape)
        out[lo] = np.where(kind <= 1, st[lo], -np.inf)
        out[hi] = np.where((kind == 0) | (kind == 2), st[hi], np.inf)
    return out


def handle(hip, st, ks, bounds):
    bs = hip.BatchSparseSolver(kkt_solver=ks) if bounds is None else hip.BatchSparseSolver(kkt_solver=ks, bounds=bounds)
    assert bs.setup(st["P"], st["Pv"], st["c"], st["A"], st["Av"], st["b"], st["G"], st["Gv"], st["h_l"], st["h_u"], st["x_l"], st["x_u"])
    return bs


def med_spread(v):
    m = float(np.median(v))
    return m, 100.0 * (max(v) - min(v)) / m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shared-only", action="store_true")
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    import torch

    import piqp_amd as hip
    parent = {}
    if args.parent:
        name = None
        for line in open(args.parent):
            if line.startswith("input: "):
                name = line[7:].strip()
            m = re.match(r"\s*\(a\) shared\s+solve kernel\s+([0-9.]+) ms \(spread ([0-9.]+)%\)", line)
            if m and name:
                parent[name] = (float(m.group(1)), float(m.group(2)))
    print(f"# bound sets of the batched sparse solver; medians over {ROUNDS} alternating rounds of the solve kernel's hipEvent time; update = wall time of "
          "update(h_l, h_u, x_l, x_u) from device tensors")
    holds_all = True
    for name, st, ks in inputs():
        cases = [("(a) shared", handle(hip, st, ks, None if args.shared_only else "shared"), st)]
        if not args.shared_only:
            mx = mixed(st, 7)
            cases += [("(b) per instance", handle(hip, st, ks, "per_instance"), st), ("(c) mixed", handle(hip, mx, ks, "per_instance"), mx)]
        for _, bs, _ in cases:  # warm-up; the second solve also fixes the start order
            bs.solve(); bs.solve()
        ms = [[] for _ in cases]
        for _ in range(ROUNDS):
            for k, (_, bs, _) in enumerate(cases):
                bs.solve()
                ms[k].append(bs.last_kernel_ms()[0])
        dev = [{k: torch.tensor(s[k], dtype=torch.float64, device="cuda:0") for k in BOUNDS if s[k] is not None} for _, _, s in cases]
        torch.cuda.synchronize()
        up = [[] for _ in cases]
        for _ in range(ROUNDS + 1):
            for k, (_, bs, _) in enumerate(cases[:2]):
                t = time.perf_counter()
                bs.update(**dev[k])
                up[k].append(1e3 * (time.perf_counter() - t))
        print(f"input: {name}")
        B = cases[0][1].batch
        for k, (label, bs, _) in enumerate(cases):
            bs.solve()
            it = bs.iterations()
            m, sp = med_spread(ms[k])
            line = f"  {label:16s} solve kernel {m:8.3f} ms (spread {sp:.1f}%)   {int((bs.statuses() == 1).sum())} of {B} solved, iterations {it.min()} .. {it.max()} (mean {it.mean():.1f}), {bs.last_kernel_ms()[1]} threads per QP"
            if k < 2:
                line += f"   update(bounds) wall {float(np.median(up[k][1:])):7.3f} ms"
            print(line)
        a = med_spread(ms[0])[0]
        if not args.shared_only:
            b, c = med_spread(ms[1])[0], med_spread(ms[2])[0]
            same = all(np.array_equal(cases[0][1].result(f), cases[1][1].result(f)) for f in ("x", "y", "z_l", "z_u", "z_bl", "z_bu"))
            print(f"  (b) / (a) = {b / a:.3f}, (c) / (a) = {c / a:.3f}; update (b) / (a) = {np.median(up[1][1:]) / np.median(up[0][1:]):.2f}   (recorded, not gated); results of (a) and (b) bitwise equal: {same}")
        if name in parent:
            pm, ps = parent[name]
            holds = a <= pm * (1 + ps / 100.0)
            holds_all &= holds
            print(f"  parent           solve kernel {pm:8.3f} ms (spread {ps:.1f}%)   (a) / parent = {a / pm:.3f}   condition (a) <= parent (1 + its spread): {'holds' if holds else 'FAILS'}")
        sys.stdout.flush()
    if parent:
        print(f"# condition ((a) not slower than the parent by more than the parent's spread, at both inputs): {'holds' if holds_all else 'FAILS'}")


if __name__ == "__main__":
    main()
