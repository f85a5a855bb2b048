#!/usr/bin/env python3
"""What BatchSparseSolver.setup() costs from host arrays and from torch CUDA tensors (pq_batch_setup_sparse_mem), beside the parent commit's setup() and a clone().
    python tools/batch_setup_timing.py --parent-lib <libpiqp_amd.so of the parent commit> > profiles/batch_setup_timing.txt
    PIQP_AMD_DEBUG=batch_setup_ms_ingest python tools/batch_setup_timing.py --ingest >> profiles/batch_setup_timing.txt
The two inputs of tools/batch_bounds_timing.py: C4 (qp_gen.mpc_batch(8192), sparse_multistage) and the sparse benchmark recipe at dim 64, 4096 QPs, sparse_ldlt;
default settings.  Per input, medians over ROUNDS alternating rounds in one process, each round: setup() of the host arrays on one handle, setup() of the same data as
CUDA tensors on a second, the parent library's pq_batch_setup_sparse of the host arrays on a third and its pq_batch_setup_sparse_mem of the same tensors on a fourth
(its own library, loaded beside this one), clone() of the device-fed handle.  The tensors are made once, before the rounds: producing them is the caller's business,
not the setup's.
  wall       the time of the Python call
  analysis   pq_batch_setup_ms[1]: symbolic analysis, entry maps, descriptor and tables on the host -- the same code in both modes
  device     pq_batch_setup_ms[2]: the handle's events from the fill of the arena (host mode: from the upload of the staging buffer) to the end of equilibration and prepare
  rest       wall - analysis - device: allocation, the fetch and the check (device mode); allocation, the host check and the upload (host mode); the wrapper.  In host mode the
             device interval is open while the host analysis runs, so the difference comes out near zero there
--ingest (run under PIQP_AMD_DEBUG=batch_setup_ms_ingest, which ends the device interval after the ingest kernels): the bytes those kernels read and write,
2 x pq_batch_last_ingest[1], over that time, beside pq_microbench_hbm_copy of the same run.
Before the rounds, with --parent-lib: the same bits as the parent.  Host-fed handles of both libraries on the shapes of tests/test_batch_setup_mem_gpu.py's twins
(SAME_BITS), both backends, the bound mode each batch is made for: equal arena strides, every arena row bitwise equal, x bitwise equal after a solve -- asserted.
Two conditions hold whatever the numbers are: the host-fed setup of this commit at most the parent's median times (1 + the parent's own spread over its rounds), and
the device-fed setup of this commit within the parent's device-fed spread in the same way.  No ratio is fixed in advance."""
import argparse
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
from batch_bounds_timing import ROUNDS, inputs, med_spread  # noqa: E402

KEYS = ("Pv", "c", "Av", "b", "Gv", "h_l", "h_u", "x_l", "x_u")


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def setup_args(st, conv):
    return (st["P"], conv(st["Pv"]), conv(st["c"]), st["A"], conv(st["Av"]), conv(st["b"]), st["G"], conv(st["Gv"]), conv(st["h_l"]), conv(st["h_u"]), conv(st["x_l"]),
            conv(st["x_u"]))


class ParentSetup:
    """pq_batch_setup_sparse(_mem) of another build of the library (the parent commit's), on a handle of its own, with this commit's argument handling"""

    def __init__(self, path, ks, bounds="shared"):
        vp = C.c_void_p
        self.L = L = C.CDLL(path)
        L.pq_batch_create.argtypes = [C.POINTER(vp), C.c_int]
        L.pq_batch_destroy.argtypes = [vp]
        L.pq_batch_destroy.restype = None
        L.pq_batch_settings.argtypes = [vp]
        L.pq_batch_settings.restype = C.POINTER(hip._lib.Settings)
        L.pq_batch_set_bound_sets.argtypes = [vp, C.c_int]
        L.pq_batch_setup_sparse.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 15
        L.pq_batch_setup_sparse_mem.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 15 + [C.c_int]
        L.pq_batch_arena_stride.argtypes = [vp]
        L.pq_batch_arena_stride.restype = C.c_longlong
        L.pq_batch_arena_row.argtypes = [vp, C.c_int, vp]
        L.pq_batch_solve.argtypes = [vp]
        L.pq_batch_get_result.argtypes = [vp, C.c_int, vp]
        self.h = vp()
        assert L.pq_batch_create(C.byref(self.h), 0) == 0
        L.pq_batch_settings(self.h).contents.kkt_solver = int(ks)
        assert L.pq_batch_set_bound_sets(self.h, 1 if bounds == "per_instance" else 0) == 0

    def setup(self, st, tensors=None):
        """st: the host arrays; tensors: the same data as CUDA tensors, in the order of KEYS (None where absent) -- then the parent's device mode"""
        pat = hip.BatchSparseSolver._pattern
        (Pp, Pi, Pm), (Ap, Ai, Am), (Gp, Gi, Gm) = pat(st["P"]), pat(st["A"]), pat(st["G"])
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        adr = (lambda a: a.ctypes.data) if tensors is None else (lambda a: a.data_ptr())
        v = dict(zip(KEYS, [f(st[k]) for k in KEYS] if tensors is None else tensors))
        if Am is None:
            v["Av"] = v["b"] = None
        if Gm is None:
            v["Gv"] = v["h_l"] = v["h_u"] = None
        ptr = [None if a is None else adr(a) for a in (v["Pv"], v["c"], v["Av"], v["b"], v["Gv"], v["h_l"], v["h_u"], v["x_l"], v["x_u"])]
        idx = [None if a is None else a.ctypes.data for a in (Pp, Pi, Ap, Ai, Gp, Gi)]
        args = [idx[0], idx[1], ptr[0], ptr[1], idx[2], idx[3], ptr[2], ptr[3], idx[4], idx[5]] + ptr[4:]
        self.B, self.n = st["c"].shape
        dims = (self.B, self.n, 0 if Am is None else Am.shape[0], 0 if Gm is None else Gm.shape[0])
        if tensors is None:
            assert self.L.pq_batch_setup_sparse(self.h, *dims, *args) == 1
        else:
            assert self.L.pq_batch_setup_sparse_mem(self.h, *dims, *args, 1) == 1

    def arena_stride(self):
        return int(self.L.pq_batch_arena_stride(self.h))

    def arena_row(self, i):
        out = np.zeros(max(self.arena_stride(), 1))
        assert self.L.pq_batch_arena_row(self.h, int(i), out.ctypes.data) == 0
        return out[:self.arena_stride()]

    def solve_x(self):
        solved = self.L.pq_batch_solve(self.h)
        assert solved >= 0
        x = np.zeros((self.B, self.n))
        assert self.L.pq_batch_get_result(self.h, 0, x.ctypes.data) == 0
        return solved, x

    def close(self):
        self.L.pq_batch_destroy(self.h)


# the shapes of the twins of tests/test_batch_setup_mem_gpu.py: (generator, dim, B, the bound mode the batch is made for)
SAME_BITS = [("random", 16, 1, "shared"), ("random", 16, 5, "shared"), ("random", 33, 5, "shared"), ("random", 33, 67, "shared"), ("mixed", 16, 8, "per_instance")]


def same_bits_as_parent(path):
    """host-fed handles of this library and of the parent's on the same data: the arena after setup() and x after solve(), bit for bit (asserted)"""
    from batch_sparse_mixed import mixed_sparse_batch
    from test_batch_ldlt_gpu import _random_sparse_qp_batch
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    rows = 0
    for kind, dim, B, bounds in SAME_BITS:
        st = _random_sparse_qp_batch(dim, B, seed=dim) if kind == "random" else mixed_sparse_batch(dim, B)
        for ks in (hip.SPARSE_MULTISTAGE, hip.SPARSE_LDLT):
            s = hip.BatchSparseSolver(kkt_solver=ks, bounds=bounds)
            assert s.setup(*setup_args(st, lambda a: a))
            par = ParentSetup(path, ks, bounds)
            par.setup(st)
            assert s.arena_stride() == par.arena_stride() > 0, (kind, dim, B, ks, s.arena_stride(), par.arena_stride())
            for i in range(B):
                assert np.array_equal(bits(s.arena_row(i)), bits(par.arena_row(i))), (kind, dim, B, ks, "arena row", i)
            solved, x = par.solve_x()
            assert s.solve() == solved and np.array_equal(bits(s.result("x")), bits(x)), (kind, dim, B, ks, "x after a solve")
            rows += B
            par.close()
    print(f"# same bits as the parent commit, host-fed setup(): {len(SAME_BITS)} shapes ({', '.join(f'{k} dim {d} B {B} {b}' for k, d, B, b in SAME_BITS)}) x sparse_multistage,"
          f" sparse_ldlt: arena strides equal, all {rows} arena rows bitwise equal, x bitwise equal after a solve: True")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ingest", action="store_true")
    args = ap.parse_args()
    import torch
    L = hip._lib.load()
    gb = C.c_double(0.0)
    assert L.pq_microbench_hbm_copy(0, 512 << 20, 20, C.byref(gb)) == 0
    on_gpu = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    if args.ingest:
        assert "batch_setup_ms_ingest" in os.environ.get("PIQP_AMD_DEBUG", ""), "run under PIQP_AMD_DEBUG=batch_setup_ms_ingest"
        print(f"# the ingest kernels of a device-fed setup alone (PIQP_AMD_DEBUG=batch_setup_ms_ingest); medians over {ROUNDS} rounds")
        print(f"# pq_microbench_hbm_copy (512 MiB): {gb.value:.0f} GB/s read + write")
        for name, st, ks in inputs():
            d = hip.BatchSparseSolver(kkt_solver=ks)
            dev = setup_args(st, on_gpu)
            torch.cuda.synchronize()
            ms = []
            for _ in range(ROUNDS + 1):
                assert d.setup(*dev)
                ms.append(d.setup_ms()["device_ms"])
            m, sp = med_spread(ms[1:])
            gbytes = 2 * d.last_ingest()["kernel_bytes"] / 1e9
            print(f"input: {name}: ingest kernels {m:8.3f} ms (spread {sp:.1f}%)   {gbytes:.3f} GB read + written   {gbytes / (1e-3 * m):6.0f} GB/s"
                  f" ({100 * gbytes / (1e-3 * m) / gb.value:.0f}% of the copy)")
            sys.stdout.flush()
        return 0
    print(f"# BatchSparseSolver.setup() from host arrays and from CUDA tensors, default settings; medians over {ROUNDS} alternating rounds; ms are per batch")
    print(f"# pq_microbench_hbm_copy (512 MiB): {gb.value:.0f} GB/s read + write")
    if args.parent_lib:
        same_bits_as_parent(args.parent_lib)
    ok_host = ok_dev = True
    for name, st, ks in inputs():
        h, d = hip.BatchSparseSolver(kkt_solver=ks), hip.BatchSparseSolver(kkt_solver=ks)
        par = ParentSetup(args.parent_lib, ks) if args.parent_lib else None
        pard = ParentSetup(args.parent_lib, ks) if args.parent_lib else None
        host, dev = setup_args(st, lambda a: a), setup_args(st, on_gpu)
        tensors = [on_gpu(st[k]) for k in KEYS]
        torch.cuda.synchronize()
        # warm-up: the kernels of both entries, the clone's gathers
        assert h.setup(*host) and d.setup(*dev)
        if par:
            par.setup(st)
            pard.setup(st, tensors)
        d.clone()
        rec = {k: [] for k in ("host", "host_an", "host_dev", "dev", "dev_an", "dev_dev", "parent", "parent_dev", "clone")}
        for _ in range(ROUNDS):
            t, ok = timed(lambda: h.setup(*host))
            assert ok
            rec["host"].append(t); rec["host_an"].append(h.setup_ms()["analysis_ms"]); rec["host_dev"].append(h.setup_ms()["device_ms"])
            t, ok = timed(lambda: d.setup(*dev))
            assert ok
            rec["dev"].append(t); rec["dev_an"].append(d.setup_ms()["analysis_ms"]); rec["dev_dev"].append(d.setup_ms()["device_ms"])
            if par:
                t, _ = timed(lambda: par.setup(st))
                rec["parent"].append(t)
                t, _ = timed(lambda: pard.setup(st, tensors))
                rec["parent_dev"].append(t)
            t, c = timed(d.clone)
            rec["clone"].append(t)
            del c
        B = h.batch
        assert h.solve() == d.solve() and np.array_equal(h.result("x"), d.result("x")), "the twins must agree bit for bit"
        med = {k: float(np.median(v)) for k, v in rec.items() if v}
        hi, di = h.last_ingest(), d.last_ingest()
        print(f"input: {name}: batch {B}, arena rows of {8 * h.arena_stride()} bytes; x of the two handles bitwise equal after a solve: True")
        for label, w, a, dv, ing in (("setup(host arrays) ", "host", "host_an", "host_dev", hi), ("setup(CUDA tensors)", "dev", "dev_an", "dev_dev", di)):
            print(f"  {label} wall {med[w]:8.2f} ms (spread {med_spread(rec[w])[1]:.1f}%)   analysis {med[a]:7.2f} ms ({100 * med[a] / med[w]:.0f}%)   device {med[dv]:7.3f} ms"
                  f"   rest {med[w] - med[a] - med[dv]:7.2f} ms   across the link {ing['link_bytes']} bytes, written by kernels {ing['kernel_bytes']} bytes")
        print(f"  clone() of the device-fed handle wall {med['clone']:8.3f} ms: the floor for the arena traffic   host / device = {med['host'] / med['dev']:.2f}x"
              f"   device / clone = {med['dev'] / med['clone']:.1f}x")
        if par:
            for label, mine, theirs, cond in (("setup(host arrays) ", "host", "parent", 1), ("setup(CUDA tensors)", "dev", "parent_dev", 2)):
                pm, ps = med_spread(rec[theirs])
                within = med[mine] <= pm * (1 + ps / 100)
                if cond == 1:
                    ok_host = ok_host and within
                else:
                    ok_dev = ok_dev and within
                print(f"  parent commit {label} wall {pm:8.2f} ms (spread {ps:.1f}%)   this commit / parent = {med[mine] / pm:.3f}"
                      f"   condition {cond}, this commit <= parent (1 + its spread): {'holds' if within else 'DOES NOT HOLD'}")
            par.close()
            pard.close()
        sys.stdout.flush()
        del h, d
    said = lambda ok: ("holds" if ok else "DOES NOT HOLD") if args.parent_lib else "not measured (no --parent-lib)"
    print(f"# condition 1 (host-fed against the parent's) at both inputs: {said(ok_host)}; condition 2 (device-fed against the parent's) at both inputs: {said(ok_dev)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
