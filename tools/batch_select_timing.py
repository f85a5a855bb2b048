#!/usr/bin/env python3
"""What acting on a list of instances in place costs (BatchSparseSolver.solve / update / result with instances=...), and what the list parameter of the
per-instance kernels costs the whole-batch calls.
    python tools/batch_select_timing.py --whole-only [--tree DIR]      (the whole-batch calls alone: nothing the parent commit lacks)
    python tools/batch_select_timing.py [--parent FILE --parent FILE]   (the whole-batch calls, the condition against the parent's outputs, then the calls by list)
profiles/batch_select_timing.txt holds the outputs in the order they ran.
The input is C4: qp_gen.mpc_batch(8192), n = 120, sparse_multistage, default settings.  Every figure is the median of ROUNDS = 7 alternating rounds in one process.

--whole-only: per round solve(), update(b) from a device tensor, update_data(P_values, A_values) from device tensors, in that order; the solve's figure is
pq_batch_last_kernel_ms (the hipEvent time of the kernel), the two updates' the wall time of the Python call (they end with a wait).  --tree DIR imports piqp_amd
from another checkout (the parent commit's, built), so the same file times both.  The parent is run twice, before and after this commit's run, in processes of its
own in the same session: its two medians and the spreads over its rounds say how far the parent is from itself.  The condition stated with --parent: this commit's
median lies inside [min, max] of the parent's two medians widened by the larger of the parent's two spreads.  No threshold beyond the parent's own spread.

By list, for count = 1, 64, 1024, 8192 (a fixed random subset, ascending; 8192: the identity): per round
  solve(instances)            kernel (pq_batch_last_kernel_ms) and wall
  update(instances, b)        wall, b a [count, p] device tensor
  result('x', instances)      wall, to a device tensor and to a host array
  clone(instances) + solve() + result('x') of the clone      wall of the three calls together, the clone released inside the interval's end
A solve by list of count = 8192 is the whole solve with one more upload; the whole solve() is beside it."""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 7
COUNTS = (1, 64, 1024, 8192)
WHOLE = ("solve kernel", "update(b) wall", "update_data(P, A) wall")


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def med_spread(v):
    import numpy as np
    m = float(np.median(v))
    return m, 100.0 * (max(v) - min(v)) / m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout piqp_amd is imported from")
    ap.add_argument("--label", default=None)
    ap.add_argument("--parent", action="append", default=[], help="an output of --whole-only --tree <the parent commit's checkout>")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch

    import piqp_amd as hip
    from qp_gen import mpc_batch
    assert os.path.abspath(os.path.dirname(os.path.dirname(hip.__file__))) == os.path.abspath(args.tree), hip.__file__

    mb = mpc_batch(8192)
    bs = hip.BatchSparseSolver(kkt_solver=hip.SPARSE_MULTISTAGE)
    assert bs.setup(mb["P_pattern"], mb["P_values"], mb["c"], mb["A_pattern"], mb["A_values"], mb["b"], x_l=mb["x_l"], x_u=mb["x_u"])
    B = bs.batch
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    b_d, P_d, A_d = dev(mb["b"]), dev(mb["P_values"]), dev(mb["A_values"])
    torch.cuda.synchronize()
    solved = bs.solve()
    bs.solve()  # (the second solve fixes the start order)
    bs.update(b=b_d); bs.update_data(P_values=P_d, A_values=A_d); bs.solve(); bs.solve()  # warm-up of the update kernels
    label = args.label or ("this commit" if os.path.abspath(args.tree) == ROOT else "parent")
    print(f"# whole-batch calls, C4 (mpc_batch(8192), n = {bs.n}, sparse_multistage), {label}: medians over {ROUNDS} rounds of solve(), update(b), update_data(P, A); "
          f"{solved} of {B} solved")
    rec = {k: [] for k in WHOLE}
    for _ in range(ROUNDS):
        bs.solve()
        rec[WHOLE[0]].append(bs.last_kernel_ms()[0])
        rec[WHOLE[1]].append(timed(lambda: bs.update(b=b_d))[0])
        rec[WHOLE[2]].append(timed(lambda: bs.update_data(P_values=P_d, A_values=A_d))[0])
    mine = {}
    for k in WHOLE:
        mine[k] = med_spread(rec[k])
        print(f"  whole {k:24s} {mine[k][0]:9.4f} ms (spread {mine[k][1]:.1f}%)")
    sys.stdout.flush()
    if args.parent:
        runs = []
        for f in args.parent:
            got = {}
            for line in open(f):
                m = re.match(r"\s*whole (.+?)\s+([0-9.]+) ms \(spread ([0-9.]+)%\)", line)
                if m:
                    got[m.group(1).strip()] = (float(m.group(2)), float(m.group(3)))
            runs.append(got)
        holds_all = True
        for k in WHOLE:
            ms = [r[k][0] for r in runs if k in r]
            sp = max(r[k][1] for r in runs if k in r)
            lo, hi = min(ms) * (1 - sp / 100.0), max(ms) * (1 + sp / 100.0)
            holds = lo <= mine[k][0] <= hi
            holds_all &= holds or mine[k][0] < lo
            print(f"  {k:24s} parent runs {', '.join(f'{m:.4f}' for m in ms)} ms, largest spread {sp:.1f}%: [{lo:.4f}, {hi:.4f}] ms; this commit {mine[k][0]:.4f} ms = "
                  f"{mine[k][0] / (sum(ms) / len(ms)):.3f} of their mean: {'inside' if holds else ('BELOW' if mine[k][0] < lo else 'ABOVE')}")
        print(f"# whole-batch calls inside the parent's own spread (or below it): {'yes' if holds_all else 'NO'}")
    if args.whole_only:
        return 0

    print(f"# by list, medians over {ROUNDS} rounds; ms per call; clone path = clone(instances) + solve() + result('x') on the clone")
    rng = np.random.default_rng(8192)
    bs.update(b=b_d)  # (the stored b of every instance is now b times its scaling, the bits an update by list writes: update_data's unscale and rescale round twice)
    bs.solve()
    x_whole = bs.result("x")
    whole_wall = []
    for count in COUNTS:
        lst = np.arange(B) if count == B else np.sort(rng.choice(B, count, replace=False))
        bl = dev(mb["b"][lst])
        torch.cuda.synchronize()
        # warm-up: the list buffer, the gather kernel, the clone's kernels
        bs.solve(instances=lst); bs.update(instances=lst, b=bl); bs.result("x", device=True, instances=lst)
        c = bs.clone(lst); c.solve(); del c
        rec = {k: [] for k in ("sk", "sw", "up", "rd", "rh", "cl")}
        same = True
        for _ in range(ROUNDS):
            t, n_ok = timed(lambda: bs.solve(instances=lst))
            rec["sw"].append(t)
            rec["sk"].append(bs.last_kernel_ms()[0])
            rec["up"].append(timed(lambda: bs.update(instances=lst, b=bl))[0])
            rec["rd"].append(timed(lambda: bs.result("x", device=True, instances=lst))[0])
            t, xs = timed(lambda: bs.result("x", instances=lst))
            rec["rh"].append(t)
            same = same and np.array_equal(xs, x_whole[lst])

            def by_clone():
                c = bs.clone(lst)
                c.solve()
                return c.result("x")
            t, xc = timed(by_clone)
            rec["cl"].append(t)
            same = same and np.array_equal(xc, xs)
            if count == B:
                whole_wall.append(timed(bs.solve)[0])
        m = {k: float(np.median(v)) for k, v in rec.items()}
        print(f"  count {count:5d}: solve(instances) kernel {m['sk']:8.4f} ms wall {m['sw']:8.4f} ms   update(instances, b) wall {m['up']:8.4f} ms   result('x', instances) wall "
              f"{m['rd']:8.4f} ms to the device, {m['rh']:8.4f} ms to the host   in place {m['sw'] + m['rh']:8.4f} ms against the clone path {m['cl']:8.4f} ms "
              f"({m['cl'] / (m['sw'] + m['rh']):.2f}x)   x of both paths bitwise the whole solve's: {same}")
        sys.stdout.flush()
    print(f"  whole solve() wall {float(np.median(whole_wall)):8.4f} ms, kernel {mine[WHOLE[0]][0]:8.4f} ms (beside count {B})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
