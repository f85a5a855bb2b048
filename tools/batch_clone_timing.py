#!/usr/bin/env python3
"""What BatchSparseSolver.clone() costs next to the only other way to a second set-up handle, setup() of the same data.
    python tools/batch_clone_timing.py > profiles/batch_clone_timing.txt
The two inputs of tools/batch_bounds_timing.py: C4 (qp_gen.mpc_batch(8192), sparse_multistage) and the sparse benchmark recipe at dim 64, 4096 QPs, sparse_ldlt;
default settings; host arrays (NumPy) for setup().  Per input, medians over ROUNDS alternating rounds in one process, each round: clone() of the set-up and solved
source, solve() of that clone, solve() of the source, clone(a fixed permutation of the batch), setup() of the same data on a second handle.  The clones of a round are
released before the next one.
  wall     the time of the Python call
  device   what pq_batch_clone_ms reports: the hipEvent time of the gathers -- the arena and the four small per-instance arrays (8 bytes, one pq_info, 64 bytes per
           instance), which ride in that time; wall minus device is the allocation of the new arena, the upload of the list and the waits
  rate     the arena's bytes read plus written (2 x 8 x batch x pq_batch_arena_stride) over that device time, beside pq_microbench_hbm_copy of the same run
  solve    pq_batch_last_kernel_ms, the hipEvent time of the solve kernel, of the whole clone and of the source; the margin is the source's spread over its rounds.
           Beside it the second solve of the same clone and the second solve of the handle that setup() made in the same round: the source's arena was allocated
           once, before everything else, theirs in this round
setup() is a host check, an upload, host analysis and several launches: wall time only.  The source's solve kernel against the parent commit is
the business of tools/batch_bounds_timing.py --shared-only, run on both trees beside this tool.  No ratio is fixed in advance."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import piqp_amd as hip  # noqa: E402
from batch_bounds_timing import ROUNDS, handle, inputs  # noqa: E402


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    L = hip._lib.load()
    gb = C.c_double(0.0)
    assert L.pq_microbench_hbm_copy(0, 512 << 20, 20, C.byref(gb)) == 0
    print(f"# BatchSparseSolver.clone() against setup() of the same data, default settings; medians over {ROUNDS} alternating rounds; ms are per batch")
    print(f"# pq_microbench_hbm_copy (512 MiB): {gb.value:.0f} GB/s read + write")
    below = True
    for name, st, ks in inputs():
        s, other = handle(hip, st, ks, None), handle(hip, st, ks, None)
        B = s.batch
        perm = np.random.default_rng(B + 3).permutation(B)
        solved = s.solve()
        s.solve()  # (the second solve fixes the start order)
        w = s.clone()  # warm-up of the gather kernels and of the clone's solve
        w.solve()
        del w
        setup_args = (st["P"], st["Pv"], st["c"], st["A"], st["Av"], st["b"], st["G"], st["Gv"], st["h_l"], st["h_u"], st["x_l"], st["x_u"])
        rec = {k: [] for k in ("cw", "cd", "pw", "pd", "setup", "src", "cl", "cl2", "oth2")}
        same = True
        for _ in range(ROUNDS):
            t, c = timed(s.clone)
            rec["cw"].append(t)
            rec["cd"].append(c.clone_ms()["device_ms"])
            assert c.solve() == solved
            rec["cl"].append(c.last_kernel_ms()[0])
            same = same and np.array_equal(c.result("x"), s.result("x"))
            c.solve()
            rec["cl2"].append(c.last_kernel_ms()[0])
            del c
            s.solve()
            rec["src"].append(s.last_kernel_ms()[0])
            t, c = timed(lambda: s.clone(perm))
            rec["pw"].append(t)
            rec["pd"].append(c.clone_ms()["device_ms"])
            del c
            t, _ = timed(lambda: other.setup(*setup_args))
            rec["setup"].append(t)
            other.solve()
            other.solve()  # (the first solve after a setup starts in index order; the second as the source and its clone do)
            rec["oth2"].append(other.last_kernel_ms()[0])
        med = {k: float(np.median(v)) for k, v in rec.items()}
        spread = max(rec["src"]) - min(rec["src"])
        gbytes = 2 * 8 * B * s.arena_stride() / 1e9
        below = below and med["cw"] < med["setup"] and med["pw"] < med["setup"]
        print(f"input: {name}: {solved} of {B} solved; arena rows of {8 * s.arena_stride()} bytes, {gbytes:.3f} GB read + written per clone")
        for label, w_, d_ in (("clone()           ", "cw", "cd"), ("clone(permutation)", "pw", "pd")):
            rate = gbytes / (1e-3 * med[d_])
            print(f"  {label} wall {med[w_]:9.3f} ms   device {med[d_]:8.3f} ms   allocation and host {med[w_] - med[d_]:8.3f} ms   gather {rate:6.0f} GB/s"
                  f" ({100 * rate / gb.value:.0f}% of the copy)   setup() wall {med['setup']:9.2f} ms   setup / clone = {med['setup'] / med[w_]:.1f}x"
                  + ("" if med[w_] < med["setup"] else "   the clone is NOT below setup() here"))
        print(f"  solve kernel of the source {med['src']:8.3f} ms (spread {100 * spread / med['src']:.1f}% over its rounds)   of the whole clone {med['cl']:8.3f} ms"
              f"   clone / source = {med['cl'] / med['src']:.3f}   {'within' if abs(med['cl'] - med['src']) <= spread else 'OUTSIDE'} the source's spread"
              f"   x of the clone bitwise the source's: {same}")
        print(f"  second solve of the same clone {med['cl2']:8.3f} ms ({med['cl2'] / med['src']:.3f} of the source)   second solve of the handle that setup() made in this round"
              f" {med['oth2']:8.3f} ms ({med['oth2'] / med['src']:.3f} of the source): a handle whose arena was allocated in this round, by either call")
        sys.stdout.flush()
        del s, other
    print(f"# a clone, whole or permuted, below setup() at both inputs: {'yes' if below else 'NO'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
