#!/usr/bin/env python3
"""What the per-instance finite-bound sets of the batched DenseSolver cost (piqp_amd.BatchDenseSolver(bounds=...), pq_solver_batch_set_bound_sets).
    python tools/dense_solver_batch_bounds_timing.py [--parent FILE] >> profiles/dense_solver_batch_bounds_timing.txt
batch = 4096 feasible QPs, the data and the four shapes of tools/dense_solver_batch_timing.py (qp_batch is imported from there); kkt_solver = dense_cholesky; default
settings.  Per shape, medians over ROUNDS alternating rounds in one process, wall and device time per QP of solve() for
  (a) shared         a handle with shared sets on the uniform data (every row of G two-sided, every variable boxed on both sides): the path of every handle so far
  (b) per instance   a handle with sets per instance on the same data: the same numbers through the per-instance tables
  (c) mixed          a handle with sets per instance on the same data with the bound kinds drawn per instance as tests/batch_qp_mixed.py draws them: per row both /
                     lower / upper / neither, per variable both / lower / upper / none
and of update(h_l, h_u, x_l, x_u) with the handle's own bounds in (a) and (b).  (b) / (a) is recorded, not gated.
--parent FILE: the output of tools/dense_solver_batch_timing.py of the parent commit, run in the same session: per shape its batch wall time and its spread over its
rounds, (max - min) / median, are read from it, and the one condition is checked: (a) is not slower than the parent by more than that spread.  The script ends with a
line that says whether it held (without --parent: that it was not checked)."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import piqp_amd as hip  # noqa: E402
from dense_solver_batch_timing import BATCH, ROUNDS, SHAPES, qp_batch  # noqa: E402

BOUNDS = ("h_l", "h_u", "x_l", "x_u")


def mixed(q, seed):
    """the same data with bound kinds per instance"""
    rng = np.random.default_rng(seed)
    b, m = q["h_l"].shape
    n = q["x_l"].shape[1]
    row, var = rng.integers(0, 4, (b, m)), rng.integers(0, 4, (b, n))
    out = dict(q)
    out["h_l"] = np.where(row <= 1, q["h_l"], -np.inf)
    out["h_u"] = np.where((row == 0) | (row == 2), q["h_u"], np.inf)
    out["x_l"] = np.where(var <= 1, q["x_l"], -np.inf)
    out["x_u"] = np.where((var == 0) | (var == 2), q["x_u"], np.inf)
    return out


def parent_figures(path):
    """{(n, p, m): (batch wall us, spread)} from the output of tools/dense_solver_batch_timing.py"""
    out, shape = {}, None
    for line in open(path):
        s = re.match(r"n = (\d+), p = (\d+), m = (\d+):", line)
        if s:
            shape = tuple(int(x) for x in s.groups())
        w = re.match(r"\s+batch\s+wall\s+([\d.]+) us \(spread ([\d.]+)%\)", line)
        if w and shape:
            out[shape] = (float(w.group(1)), float(w.group(2)) / 100)
    return out


def main():
    parent = parent_figures(sys.argv[sys.argv.index("--parent") + 1]) if "--parent" in sys.argv else None
    print(f"# bound sets of the batched DenseSolver, {BATCH} QPs per handle, kkt_solver = dense_cholesky, default settings; medians over {ROUNDS} alternating rounds; us are per QP")
    held = True
    for n, p, m in SHAPES:
        q = qp_batch(n, p, m, BATCH, 1000 * n + 10 * p + m)
        data = dict(a=q, b=q, c=mixed(q, 7919 * (1000 * n + 10 * p + m)))
        handles = dict(a=hip.BatchDenseSolver(bounds="shared"), b=hip.BatchDenseSolver(bounds="per_instance"), c=hip.BatchDenseSolver(bounds="per_instance"))
        solved = {}
        for k, s in handles.items():
            s.setup(**data[k])
            solved[k] = s.solve()  # warm-up
        rec = {f"{k}_{w}": [] for k in handles for w in ("wall", "dev")}
        rec.update({f"{k}_{w}": [] for k in "ab" for w in ("uwall", "udev")})
        for _ in range(ROUNDS):
            for k, s in handles.items():
                s.solve()
                ms = s.last_ms()
                rec[f"{k}_wall"].append(1e3 * ms["wall_ms"] / BATCH)
                rec[f"{k}_dev"].append(1e3 * ms["device_ms"] / BATCH)
            for k in "ab":
                handles[k].update(**{v: q[v] for v in BOUNDS})
                ms = handles[k].last_update_ms()
                rec[f"{k}_uwall"].append(1e3 * ms["wall_ms"] / BATCH)
                rec[f"{k}_udev"].append(1e3 * ms["device_ms"] / BATCH)
        med = {k: float(np.median(v)) for k, v in rec.items()}
        spread = {k: (max(rec[f"{k}_wall"]) - min(rec[f"{k}_wall"])) / med[f"{k}_wall"] for k in handles}
        same = all(np.array_equal(handles["a"].result(nm).view(np.uint64), handles["b"].result(nm).view(np.uint64)) for nm in ("x", "y", "z_l", "z_u", "z_bl", "z_bu"))
        it = {k: s.iterations() for k, s in handles.items()}
        print(f"n = {n}, p = {p}, m = {m}: solved {solved['a']} / {solved['b']} / {solved['c']} of {BATCH}; results of (a) and (b) bitwise equal: {same}")
        for k, name in (("a", "(a) shared      "), ("b", "(b) per instance"), ("c", "(c) mixed       ")):
            print(f"  {name} solve wall {med[f'{k}_wall']:9.2f} us (spread {100 * spread[k]:.1f}%)   device {med[f'{k}_dev']:9.2f} us   iterations {it[k].min()} .. {it[k].max()}"
                  f" (mean {it[k].mean():.1f})" + (f"   update(bounds) wall {med[f'{k}_uwall']:7.3f} us   device {med[f'{k}_udev']:7.3f} us" if k in "ab" else ""))
        print(f"  (b) / (a): solve wall {med['b_wall'] / med['a_wall']:.3f}, device {med['b_dev'] / med['a_dev']:.3f}; update wall {med['b_uwall'] / med['a_uwall']:.3f},"
              f" device {med['b_udev'] / med['a_udev']:.3f}   (recorded, not gated)")
        if parent is not None:
            pw, ps = parent[(n, p, m)]
            ok = med["a_wall"] <= pw * (1 + ps)
            held = held and ok
            print(f"  parent   solve wall {pw:9.2f} us (spread {100 * ps:.1f}%)   (a) / parent = {med['a_wall'] / pw:.3f}   condition (a) <= parent (1 + its spread): {'holds' if ok else 'FAILS'}")
        del handles
    if parent is None:
        print("# condition ((a) not slower than the parent by more than the parent's spread): not checked, no --parent file")
        return 0
    print(f"# condition ((a) not slower than the parent by more than the parent's spread, at every shape): {'holds' if held else 'FAILS'}")
    return 0 if held else 1


if __name__ == "__main__":
    sys.exit(main())
