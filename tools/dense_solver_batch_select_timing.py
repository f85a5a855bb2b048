#!/usr/bin/env python3
"""What acting on a list of instances in place costs (BatchDenseSolver.solve / update / result with instances=...), and what the list parameter of the per-instance
kernels costs the whole-batch calls.
    python tools/dense_solver_batch_select_timing.py --whole-only [--tree DIR]      (the whole-batch calls alone: nothing the parent commit lacks)
    python tools/dense_solver_batch_select_timing.py [--parent FILE --parent FILE]   (the whole-batch calls, the condition against the parent's outputs, the calls by list)
    python tools/dense_solver_batch_select_timing.py --compare FILE --parent FILE --parent FILE   (no GPU: the condition, from an output of this commit and the parent's two)
profiles/dense_solver_batch_select_timing.txt holds the outputs in the order they ran.
batch = 4096 QPs at the four shapes and with the inputs of tools/dense_solver_batch_timing.py; kkt_solver = dense_cholesky; default settings.  Every figure is the
median of ROUNDS = 7 alternating rounds in one process.

--whole-only: per shape and round solve(), update(c, b) from device tensors ("vectors"), update(all nine arguments) from device tensors ("all"), in that order: wall
time of the Python call and the device time the handle reports (pq_solver_batch_last_ms, pq_solver_batch_last_update_ms).  --tree DIR imports piqp_amd from another
checkout (the parent commit's, built), so the same file times both.  The parent is run twice, before and after this commit's run, in processes of its own in the same
session: its two medians and the spreads over its rounds say how far the parent is from itself.  The condition stated with --parent: this commit's median lies inside
[min, max] of the parent's two medians widened by the larger of the parent's two spreads.  No threshold beyond the parent's own spread.

By list, for count = 1, 64, 1024 (a fixed random subset, ascending): per round
  solve(instances)              wall and device
  update(c, b, instances)       wall and device, c and b [count, len] device tensors
  result('x', instances)        wall, to a device tensor and to a host array
  the same through clone(instances): clone + update(c, b) + solve() + result('x') of the clone, wall of the four calls together, the clone released inside the interval
The whole solve() is beside them.  No factor is claimed in advance; what comes out is printed, a loss included."""
# (bitwise equality of the calls by list with the whole-batch calls is the business of tests/test_dense_solver_batch_select_gpu.py; here the x of both paths is only held
# against the whole solve's to solver accuracy)
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 64, 1024)
WHOLE = ("solve wall", "solve device", "update(vectors) wall", "update(vectors) device", "update(all) wall", "update(all) device")


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def med_spread(v):
    import numpy as np
    m = float(np.median(v))
    return m, 100.0 * (max(v) - min(v)) / m


def whole_lines(path):
    got = {}
    for line in open(path):
        m = re.match(r"\s*whole n = (\d+) (.+?)\s+([0-9.]+) ms \(spread ([0-9.]+)%\)", line)
        if m:
            got[(int(m.group(1)), m.group(2).strip())] = (float(m.group(3)), float(m.group(4)))
    return got


def condition(n, mine, parents):
    """prints, per whole-batch figure of shape n, where this commit's median lies against the parent's runs; returns whether every one is inside or below"""
    ok = True
    for k in WHOLE:
        ms = [r[(n, k)][0] for r in parents if (n, k) in r]
        sp = max(r[(n, k)][1] for r in parents if (n, k) in r)
        lo, hi = min(ms) * (1 - sp / 100.0), max(ms) * (1 + sp / 100.0)
        holds = lo <= mine[k][0] <= hi
        ok &= holds or mine[k][0] < lo
        print(f"  n = {n} {k:24s} parent runs {', '.join(f'{v:.4f}' for v in ms)} ms, largest spread {sp:.1f}%: [{lo:.4f}, {hi:.4f}] ms; this commit {mine[k][0]:.4f} ms = "
              f"{mine[k][0] / (sum(ms) / len(ms)):.3f} of their mean: {'inside' if holds else ('BELOW' if mine[k][0] < lo else 'ABOVE')}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--whole-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout piqp_amd is imported from")
    ap.add_argument("--label", default=None)
    ap.add_argument("--parent", action="append", default=[], help="an output of --whole-only --tree <the parent commit's checkout>")
    ap.add_argument("--compare", default=None, help="an output of this commit: print the condition against the --parent files and stop (no GPU)")
    args = ap.parse_args()
    if args.compare:
        mine, parents = whole_lines(args.compare), [whole_lines(f) for f in args.parent]
        ok = True
        for n in sorted({k[0] for k in mine}):
            ok &= condition(n, {k[1]: v for k, v in mine.items() if k[0] == n}, parents)
        print(f"# whole-batch calls inside the parent's own spread (or below it) at every shape: {'yes' if ok else 'NO'}")
        return 0
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import torch

    import piqp_amd as hip
    assert os.path.abspath(os.path.dirname(os.path.dirname(hip.__file__))) == os.path.abspath(args.tree), hip.__file__
    sys.path.append(ROOT)  # (dense_solver_batch_timing imports piqp_amd and the oracle: the first is loaded by now, the second comes from this checkout)
    from dense_solver_batch_timing import BATCH, ROUNDS, SHAPES, qp_batch

    label = args.label or ("this commit" if os.path.abspath(args.tree) == ROOT else "parent")
    parents = [whole_lines(f) for f in args.parent]
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    holds_all = True
    for n, p, m in SHAPES:
        seed = 1000 * n + 10 * p + m
        q = qp_batch(n, p, m, BATCH, seed)
        qd = {k: dev(v) for k, v in q.items()}
        torch.cuda.synchronize()
        s = hip.BatchDenseSolver()
        s.setup(**q)
        solved = s.solve()
        s.update(c=qd["c"], b=qd["b"]); s.update(**qd); s.solve()  # warm-up of the update kernels
        print(f"# n = {n}, p = {p}, m = {m}, {BATCH} QPs, {label}: medians over {ROUNDS} rounds; {solved} of {BATCH} solved")
        rec = {k: [] for k in WHOLE}
        for _ in range(ROUNDS):
            rec[WHOLE[0]].append(timed(s.solve)[0])
            rec[WHOLE[1]].append(s.last_ms()["device_ms"])
            rec[WHOLE[2]].append(timed(lambda: s.update(c=qd["c"], b=qd["b"]))[0])
            rec[WHOLE[3]].append(s.last_update_ms()["device_ms"])
            rec[WHOLE[4]].append(timed(lambda: s.update(**qd))[0])
            rec[WHOLE[5]].append(s.last_update_ms()["device_ms"])
        mine = {}
        for k in WHOLE:
            mine[k] = med_spread(rec[k])
            print(f"  whole n = {n} {k:24s} {mine[k][0]:9.4f} ms (spread {mine[k][1]:.1f}%)")
        if parents:
            holds_all &= condition(n, mine, parents)
        sys.stdout.flush()
        if args.whole_only:
            del s
            continue
        s.update(c=qd["c"], b=qd["b"])  # (the stored data of every instance are now what an update(c, b) leaves: the bits an update by list writes again)
        s.solve()
        x_whole = s.result("x")
        rng = np.random.default_rng(seed + 7)
        for count in COUNTS:
            lst = np.sort(rng.choice(BATCH, count, replace=False))
            cl, bl = dev(q["c"][lst]), dev(q["b"][lst])
            torch.cuda.synchronize()
            # warm-up: the list buffer, the scatter and gather kernels, the clone's kernels
            s.update(c=cl, b=bl, instances=lst); s.solve(instances=lst); s.result("x", device=True, instances=lst)
            c = s.clone(lst); c.update(c=cl, b=bl); c.solve(); del c
            rec = {k: [] for k in ("uw", "ud", "sw", "sd", "rd", "rh", "cl")}
            far = 0.0  # (every update unscales and rescales the instance's data, which moves them by roundings: the x of the rounds agree to solver accuracy, not bit for bit)
            for _ in range(ROUNDS):
                rec["uw"].append(timed(lambda: s.update(c=cl, b=bl, instances=lst))[0])
                rec["ud"].append(s.last_update_ms()["device_ms"])
                rec["sw"].append(timed(lambda: s.solve(instances=lst))[0])
                rec["sd"].append(s.last_ms()["device_ms"])
                rec["rd"].append(timed(lambda: s.result("x", device=True, instances=lst))[0])
                t, xs = timed(lambda: s.result("x", instances=lst))
                rec["rh"].append(t)
                far = max(far, float(np.abs(xs - x_whole[lst]).max()))

                def by_clone():
                    c = s.clone(lst)
                    c.update(c=cl, b=bl)
                    c.solve()
                    return c.result("x")
                t, xc = timed(by_clone)
                rec["cl"].append(t)
                far = max(far, float(np.abs(xc - x_whole[lst]).max()))
            md = {k: float(np.median(v)) for k, v in rec.items()}
            place = md["uw"] + md["sw"] + md["rh"]
            print(f"  count {count:5d}: update(c, b, instances) wall {md['uw']:8.4f} ms device {md['ud']:8.4f} ms   solve(instances) wall {md['sw']:8.4f} ms device {md['sd']:8.4f} ms"
                  f"   result('x', instances) wall {md['rd']:8.4f} ms to the device, {md['rh']:8.4f} ms to the host   the three in place {place:8.4f} ms against the clone path "
                  f"{md['cl']:8.4f} ms ({md['cl'] / place:.2f}x)   max |x - x of the whole solve| over both paths {far:.1e}")
            sys.stdout.flush()
        print(f"  whole solve() wall {mine[WHOLE[0]][0]:8.4f} ms device {mine[WHOLE[1]][0]:8.4f} ms; whole update(c, b) wall {mine[WHOLE[2]][0]:8.4f} ms")
        del s
    if parents:
        print(f"# whole-batch calls inside the parent's own spread (or below it) at every shape: {'yes' if holds_all else 'NO'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
