#!/usr/bin/env python3
"""Device time of the batched KKTSystem (piqp_amd.BatchKKTSystem, pq_kktsys_batch_*) next to what stands below and beside it.
    python tools/kktsys_batch_timing.py > profiles/kktsys_batch_timing.txt
batch = 4096 instances, all different, (n, p, m) = (8, 2, 16), (32, 8, 64), (64, 16, 128), (128, 32, 256); every row of G two-sided, every variable boxed on both
sides; data and vectors resident in device memory; kkt_solver = dense_cholesky.  Three comparisons, all hipEvent times of launches unless said otherwise:
  1 factor   the ONE update_scalings_and_factor launch of the system (refinement off, and on) against the bare pq_kkt_batch_update_scalings_and_factor launch on the
             same data and the scalings the system computed, plus the scalings as stand-alone elementwise work (torch expressions over the batch: what a user of
             BatchDenseKKT alone can do; `ops` launches, timed with torch events)
  2 solve    the ONE solve launch with refinement off against the bare pq_kkt_batch_solve launch on the condensed right-hand side; with refinement on under
             iterative_refinement_static_regularization_eps = 1e-4 (so that steps are taken): the launch, the mean number of steps, and
             (launch - launch without refinement) / (batch x mean steps) as the cost of one step of one instance
  3 single   per instance, WALL time of update_scalings_and_factor + solve of a loop over 64 single pq_kktsys handles (kkt_solver = 19, host-mode vectors; the
             only way to these results without the batched system) against the batched launches' device time per instance
Medians over ROUNDS alternating rounds (of REPS calls each) in one process; spread = (max - min) / median over the rounds of the system's launch."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import piqp_amd as hip  # noqa: E402

BATCH, ROUNDS, REPS, SINGLES = 4096, 7, 3, 64
SHAPES = ((8, 2, 16), (32, 8, 64), (64, 16, 128), (128, 32, 256))
NAMES = ("x", "y", "z_l", "z_u", "z_bl", "z_bu", "s_l", "s_u", "s_bl", "s_bu")


def qp_batch(n, p, m, batch, seed):
    rng = np.random.default_rng(seed)
    U = np.triu(rng.standard_normal((batch, n, n)), 1)
    P = U + U.transpose(0, 2, 1)
    P[:, np.arange(n), np.arange(n)] = np.abs(P).sum(axis=2) + 1.0
    return P, rng.standard_normal((batch, p, n)), rng.standard_normal((batch, m, n)), rng


def torch_scalings(rho, delta, v):
    """x_reg, z_reg of kkt_system.hpp:150-193 for the pattern of this tool (every bound finite, x_b_scaling = 1) as torch expressions"""
    d = delta[:, None]
    z_reg = 1.0 / (1.0 / ((1.0 / v["z_l"]) * v["s_l"] + d) + 1.0 / ((1.0 / v["z_u"]) * v["s_u"] + d))
    x_reg = rho[:, None] + 1.0 / ((1.0 / v["z_bl"]) * v["s_bl"] + d) + 1.0 / ((1.0 / v["z_bu"]) * v["s_bu"] + d)
    return x_reg, z_reg


def torch_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    print(f"# the batched KKTSystem, {BATCH} instances per launch, kkt_solver = dense_cholesky; medians over {ROUNDS} alternating rounds of {REPS} calls; ms are launches, us per instance")
    for n, p, m in SHAPES:
        P, A, G, rng = qp_batch(n, p, m, BATCH, n)
        shapes = dict(zip(NAMES, ((BATCH, n), (BATCH, p), (BATCH, m), (BATCH, m), (BATCH, n), (BATCH, n), (BATCH, m), (BATCH, m), (BATCH, n), (BATCH, n))))
        every_row, every_var = np.arange(m, dtype=np.int32), np.arange(n, dtype=np.int32)
        mk = lambda **kw: hip.BatchKKTSystem(dev(P), dev(A), dev(G), h_l_idx=every_row, h_u_idx=every_row, x_l_idx=every_var, x_u_idx=every_var,
                                             settings=hip.default_settings(**kw))
        ks, ksB = mk(), mk(iterative_refinement_static_regularization_eps=1e-4)
        kb = hip.BatchDenseKKT(dev(P), dev(A), dev(G))
        v = {nm: 10.0 ** rng.uniform(-6, 2, shapes[nm]) if nm[0] in "sz" else np.zeros(shapes[nm]) for nm in NAMES}
        rho, delta = 10.0 ** rng.uniform(-9, -3, (2, BATCH))
        rhs = {nm: rng.standard_normal(shapes[nm]) for nm in NAMES}
        dv, drhs, drho, ddelta = {nm: dev(a) for nm, a in v.items()}, {nm: dev(a) for nm, a in rhs.items()}, dev(rho), dev(delta)
        off, on = torch.zeros(BATCH, dtype=torch.int32, device="cuda"), torch.ones(BATCH, dtype=torch.int32, device="cuda")
        out = {nm: torch.zeros(shapes[nm], dtype=torch.float64, device="cuda") for nm in NAMES}
        # what the bare backend is given: the system's own scalings and condensed right-hand side (refinement off: delta_reg = delta, z_reg_iter_ref = z_reg)
        assert ks.update_scalings_and_factor(off, drho, ddelta, dv) == BATCH
        ks.solve(drhs, out=out)
        assert ks.solve_ok().all()
        bsc = [ddelta, dev(ks.x_reg()), dev(ks.z_reg())]
        brhs = [dev(ks.rhs_x_bar()), drhs["y"], dev(ks.rhs_z_bar())]
        bout = [torch.empty_like(a) for a in brhs]
        xr, zr = torch_scalings(drho, ddelta, dv)
        assert np.allclose(xr.cpu().numpy(), ks.x_reg(), rtol=1e-12) and np.allclose(zr.cpu().numpy(), ks.z_reg(), rtol=1e-12)
        # single handles
        singles = []
        for i in range(SINGLES):
            q = dict(P=P[i], c=np.zeros(n), A=A[i], b=np.zeros(p), G=G[i], h_l=-np.ones(m), h_u=np.ones(m), x_l=-np.ones(n), x_u=np.ones(n))
            singles.append(hip.KKTSystem(hip.Data(**q), hip.default_settings(kkt_solver=hip.DENSE_CHOLESKY_EXACT)))
        rows = [({nm: np.ascontiguousarray(a[i]) for nm, a in v.items()}, {nm: np.ascontiguousarray(a[i]) for nm, a in rhs.items()}) for i in range(SINGLES)]

        def system(k, flags):
            assert k.update_scalings_and_factor(flags, drho, ddelta, dv) == BATCH
            k.solve(drhs, out=out)
            return k.last_ms()[:2]

        def bare():
            assert kb.update_scalings_and_factor(*bsc) == BATCH
            kb.solve(*brhs, out=bout)
            return kb.last_ms()[:2]

        def single_us():
            t = []
            for k1, (v1, r1) in zip(singles, rows):
                t0 = time.perf_counter()
                ok = k1.update_scalings_and_factor(False, float(rho[0]), float(delta[0]), v1)
                t1 = time.perf_counter()
                ok2, _ = k1.solve(r1)
                t2 = time.perf_counter()
                assert ok and ok2
                t.append(((t1 - t0) * 1e6, (t2 - t1) * 1e6))
            return np.median(np.array(t), axis=0)

        for _ in range(2):
            system(ks, off); system(ks, on); system(ksB, on); bare(); torch_ms(lambda: torch_scalings(drho, ddelta, dv)); single_us()
        R = dict(off=[], on=[], B=[], bare=[], ew=[], single=[])
        for _ in range(ROUNDS):
            R["off"].append(np.median([system(ks, off) for _ in range(REPS)], axis=0))
            R["bare"].append(np.median([bare() for _ in range(REPS)], axis=0))
            R["ew"].append(np.median([torch_ms(lambda: torch_scalings(drho, ddelta, dv)) for _ in range(REPS)]))
            R["on"].append(np.median([system(ks, on) for _ in range(REPS)], axis=0))
            R["B"].append(np.median([system(ksB, on) for _ in range(REPS)], axis=0))
            R["single"].append(single_us())
        system(ks, on)
        system(ksB, on)
        steps_on, steps_B = ks.refine_steps().mean(), ksB.refine_steps().mean()
        M = {k: np.median(np.array(x), axis=0) for k, x in R.items()}
        spread = (np.array(R["off"]).max(axis=0) - np.array(R["off"]).min(axis=0)) / M["off"]
        us = lambda ms: 1e3 * ms / BATCH
        print(f"n = {n}, p = {p}, m = {m}")
        print(f"  1 factor  system (refinement off) {M['off'][0]:8.3f} ms (spread {100 * spread[0]:.1f}%)   bare backend {M['bare'][0]:8.3f} ms + scalings as torch elementwise work {M['ew']:7.3f} ms"
              f" = {M['bare'][0] + M['ew']:8.3f} ms   system / (bare + elementwise) = {M['off'][0] / (M['bare'][0] + M['ew']):.2f}   system / bare = {M['off'][0] / M['bare'][0]:.2f}"
              f"   refinement on: {M['on'][0]:8.3f} ms")
        print(f"  2 solve   system (refinement off) {M['off'][1]:8.3f} ms (spread {100 * spread[1]:.1f}%)   bare backend {M['bare'][1]:8.3f} ms   system / bare = {M['off'][1] / M['bare'][1]:.2f}")
        for tag, key, st in (("default settings", "on", steps_on), ("static_regularization_eps 1e-4", "B", steps_B)):
            per = us(M[key][1] - M["off"][1]) / st if st > 0 else float("nan")
            print(f"            refinement on, {tag}: {M[key][1]:8.3f} ms, mean steps {st:.2f}, per step and instance {per:.3f} us")
        print(f"  3 single  per instance: {SINGLES} single pq_kktsys handles (kkt_solver 19), wall: factor {M['single'][0]:8.1f} us, solve {M['single'][1]:8.1f} us   "
              f"batched system, device: factor {us(M['off'][0]):.3f} us, solve {us(M['off'][1]):.3f} us   ratio {M['single'][0] / us(M['off'][0]):.0f}x, {M['single'][1] / us(M['off'][1]):.0f}x",
              flush=True)
        del ks, ksB, kb, singles


if __name__ == "__main__":
    main()
