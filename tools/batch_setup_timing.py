#!/usr/bin/env python3
"""What BatchSparseSolver.setup() costs from host arrays and from torch CUDA tensors (pq_batch_setup_sparse_mem), beside the parent commit's setup() and a clone().
    python tools/batch_setup_timing.py --parent-lib <libpiqp_amd.so of the parent commit> > profiles/batch_setup_timing.txt
    PIQP_AMD_DEBUG=batch_setup_ms_ingest python tools/batch_setup_timing.py --ingest >> profiles/batch_setup_timing.txt
The two inputs of tools/batch_bounds_timing.py: C4 (qp_gen.mpc_batch(8192), sparse_multistage) and the sparse benchmark recipe at dim 64, 4096 QPs, sparse_ldlt;
default settings.  Per input, medians over ROUNDS alternating rounds in one process, each round: setup() of the host arrays on one handle, setup() of the same data as
CUDA tensors on a second, the parent library's pq_batch_setup_sparse of the host arrays on a third (its own library, loaded beside this one), clone() of the
device-fed handle.  The tensors are made once, before the rounds: producing them is the caller's business, not the setup's.
  wall       the time of the Python call
  analysis   pq_batch_setup_ms[1]: symbolic analysis, entry maps, descriptor and tables on the host -- the same code in both modes
  device     pq_batch_setup_ms[2]: the handle's events from the fill of the arena to the end of equilibration and prepare
  rest       wall - analysis - device: allocation, the fetch and the check (device mode); HostData per instance and packing (host mode); the wrapper
--ingest (run under PIQP_AMD_DEBUG=batch_setup_ms_ingest, which ends the device interval after the ingest kernels): the bytes those kernels read and write,
2 x pq_batch_last_ingest[1], over that time, beside pq_microbench_hbm_copy of the same run.
Two conditions hold whatever the numbers are: the host-fed setup of this commit within the parent's own spread over its rounds, and the device-fed setup below the
host-fed one at both inputs.  No ratio is fixed in advance."""
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
    """pq_batch_setup_sparse of another build of the library (the parent commit's), on a handle of its own, with this commit's argument handling"""

    def __init__(self, path, ks):
        vp = C.c_void_p
        self.L = L = C.CDLL(path)
        L.pq_batch_create.argtypes = [C.POINTER(vp), C.c_int]
        L.pq_batch_destroy.argtypes = [vp]
        L.pq_batch_destroy.restype = None
        L.pq_batch_settings.argtypes = [vp]
        L.pq_batch_settings.restype = C.POINTER(hip._lib.Settings)
        L.pq_batch_setup_sparse.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 15
        self.h = vp()
        assert L.pq_batch_create(C.byref(self.h), 0) == 0
        L.pq_batch_settings(self.h).contents.kkt_solver = int(ks)

    def setup(self, st):
        pat = hip.BatchSparseSolver._pattern
        (Pp, Pi, Pm), (Ap, Ai, Am), (Gp, Gi, Gm) = pat(st["P"]), pat(st["A"]), pat(st["G"])
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        keep = [Pp, Pi, f(st["Pv"]), f(st["c"]), Ap, Ai, f(st["Av"]), f(st["b"]), Gp, Gi, f(st["Gv"]), f(st["h_l"]), f(st["h_u"]), f(st["x_l"]), f(st["x_u"])]
        ptr = [None if a is None else a.ctypes.data for a in keep]
        B, n = st["c"].shape
        assert self.L.pq_batch_setup_sparse(self.h, B, n, 0 if Am is None else Am.shape[0], 0 if Gm is None else Gm.shape[0], *ptr) == 1

    def close(self):
        self.L.pq_batch_destroy(self.h)


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
    ok_host = ok_dev = True
    for name, st, ks in inputs():
        h, d = hip.BatchSparseSolver(kkt_solver=ks), hip.BatchSparseSolver(kkt_solver=ks)
        par = ParentSetup(args.parent_lib, ks) if args.parent_lib else None
        host, dev = setup_args(st, lambda a: a), setup_args(st, on_gpu)
        torch.cuda.synchronize()
        # warm-up: the kernels of both paths, the clone's gathers
        assert h.setup(*host) and d.setup(*dev)
        if par:
            par.setup(st)
        d.clone()
        rec = {k: [] for k in ("host", "host_an", "host_dev", "dev", "dev_an", "dev_dev", "parent", "clone")}
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
        dev_below = med["dev"] < med["host"]
        ok_dev = ok_dev and dev_below
        print(f"  condition 2, device-fed below host-fed: {'holds' if dev_below else 'DOES NOT HOLD'}")
        if par:
            pm, ps = med_spread(rec["parent"])
            within = med["host"] <= pm * (1 + ps / 100)
            ok_host = ok_host and within
            print(f"  parent commit setup(host arrays) wall {pm:8.2f} ms (spread {ps:.1f}%)   this commit / parent = {med['host'] / pm:.3f}"
                  f"   condition 1, host-fed <= parent (1 + its spread): {'holds' if within else 'DOES NOT HOLD'}")
            par.close()
        sys.stdout.flush()
        del h, d
    print(f"# condition 1 at both inputs: {('holds' if ok_host else 'DOES NOT HOLD') if args.parent_lib else 'not measured (no --parent-lib)'}; condition 2 at both inputs: "
          f"{'holds' if ok_dev else 'DOES NOT HOLD'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
