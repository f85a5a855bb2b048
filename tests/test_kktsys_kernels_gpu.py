"""The non-batched KKTSystem shell (piqp_amd/csrc/kkt_system.hip behind pq_kktsys_*, piqp_amd.KKTSystem): the scalings, the reduction to the condensed right-hand side,
the refinement loop with its five exits, the dual and box recoveries, mul and the non-finite detection, held to the CPU oracle (oracle/orc_kkt_system.c) on the raw
doubles.  There is no tolerance in this file and no case is left out: equality is same() of tests/test_dense_exact_gpu.py (the uint64 views).

The cases, their inputs and the NumPy restatement of the elementwise formulas come from tests/kktsys_shapes.py; tests/test_kktsys_shapes.py asserts on the CPU that the
oracle factors and solves every one of them, leaves the refinement loop through each exit, and that the restatement is the oracle's arithmetic.  The device handle is
fed the oracle's own matrices, index lists and x_b_scaling.

1. the whole shell on the two reference-order backends (DENSE_CHOLESKY_EXACT against the oracle's dense_cholesky, SPARSE_LDLT_EXACT against its sparse_ldlt): every
   number of every step is the oracle's;
2. the shell alone on the fast backends, whose own rounding differs from the oracle's: what does not pass through the backend is the oracle's, what does is the NumPy
   restatement applied to the device's own backend results;
3. non-finite right-hand sides at every block and wave edge of every index range."""
import numpy as np
import pytest

import kktsys_shapes as ks
from qp_gen import mpc_chain, random_vars
from test_dense_exact_gpu import same

pytestmark = pytest.mark.gpu

DENSE_CHOLESKY, SPARSE_MULTISTAGE, DENSE_LDLT_NO_PIVOT, SPARSE_LDLT_EXACT, SPARSE_LDLT_MULTIFRONTAL, DENSE_CHOLESKY_EXACT = 0, 5, 16, 17, 18, 19
EXACT = [pytest.param(False, id="dense_cholesky_exact"), pytest.param(True, id="sparse_ldlt_exact")]
STATES = ("X_REG", "Z_REG", "RHS_X_BAR", "RHS_Z_BAR", "LHS_Z")
PQ_ERR_INVALID = -1  # include/piqp_amd.h


def pair(hip, orc, q, xbs, sparse, variant, dev_kind=None, orc_kind=None):
    """(oracle data, lists, device handle, oracle) of one problem under one settings variant"""
    od = ks.oracle_data(orc, q, xbs, sparse)
    d = ks.lists(od)
    dd = ks.device_data(hip, od)
    assert all(np.array_equal(getattr(dd, nm + "_idx"), getattr(d, nm)) for nm in ("h_l", "h_u", "x_l", "x_u"))
    if dev_kind is None:
        dev_kind = SPARSE_LDLT_EXACT if sparse else DENSE_CHOLESKY_EXACT
    if orc_kind is None:
        orc_kind = orc.SPARSE_LDLT if sparse else orc.DENSE_CHOLESKY
    kh = hip.KKTSystem(dd, hip.default_settings(kkt_solver=dev_kind, **ks.VARIANTS[variant]))
    ko = orc.KKTSystem(od, orc.Settings(kkt_solver=orc_kind, **ks.VARIANTS[variant]))
    return od, d, kh, ko


def reference(ko, d, inp):
    """the oracle's step, with the condensed residual of what its solve returned (what the refinement loop records of its kept iterate)"""
    R = ks.oracle_step(ko, d, *inp)
    assert R.ok_f and R.ok_s  # (tests/test_kktsys_shapes.py)
    R.residual = ks.condensed_residual(ko, d, ks.scalings(d, inp[1], inp[2], inp[3]), R.x_reg, R, inp[4])
    return R


def host(a):
    return a.cpu().numpy() if type(a).__module__.startswith("torch") else np.asarray(a)


def device(v):
    """the vectors in GPU memory, complete before the handle's stream reads them (the caller's half of the ordering contract of PQ_MEM_DEVICE)"""
    import torch
    out = {nm: torch.from_numpy(np.ascontiguousarray(a)).cuda() for nm, a in v.items()}
    torch.cuda.synchronize()
    return out


def solve_checks(kh, d, R, lhs, ok, tag):
    """what a solve leaves behind, against the oracle's"""
    bad = []
    if ok != R.ok_s:
        bad.append(("solve returned", ok))
    bad += [("lhs", nm) for nm in ks.NAMES if not same(host(lhs[nm])[:d.used[nm]], R.lhs[nm][:d.used[nm]])]
    bad += [nm for nm, ref in (("RHS_X_BAR", R.rxb), ("RHS_Z_BAR", R.rzb), ("LHS_Z", R.lhs_z)) if not same(kh.state(nm), ref)]
    st = kh.last_solve_stats()
    if (st["refine_steps"], st["backend_solves"]) != (R.steps, R.solves):
        bad.append(("steps, solves", st["refine_steps"], st["backend_solves"], R.steps, R.solves))
    if not (same(st["refine_error"], R.refine_error) and same(st["rhs_norm"], R.rhs_norm)):
        bad.append(("refine_error, rhs_norm", st["refine_error"], st["rhs_norm"], R.refine_error, R.rhs_norm))
    res, nrm = kh.condensed_residual()
    if R.exit >= 0 and not same(res, R.refine_error):
        bad.append(("condensed_residual against the oracle's last refine error", res, R.refine_error, "exit", R.exit))
    if not (same(res, R.residual[0]) and same(nrm, R.residual[1])):
        bad.append(("condensed_residual", res, nrm, R.residual))
    assert not bad, (tag, "exit", R.exit, bad)


def device_step(kh, d, inp, R, tag, torch_pointers=False):
    """the same step on the handle, every number against the oracle's"""
    refine, rho, delta, v, rhs, lhs_mul = inp
    if torch_pointers:
        v, rhs, lhs_mul = device(v), device(rhs), device(lhs_mul)
    ok_f = kh.update_scalings_and_factor(refine, rho, delta, v)
    assert ok_f == R.ok_f, (tag, "factor", ok_f)
    bad = [nm for nm, ref in (("X_REG", R.x_reg), ("Z_REG", R.z_reg)) if not same(kh.state(nm), ref)]
    assert not bad, (tag, bad)
    ok, lhs = kh.solve(rhs)
    solve_checks(kh, d, R, lhs, ok, tag)
    got = kh.mul(lhs_mul)
    kh.synchronize()  # (with device pointers mul is asynchronous on the handle's stream)
    bad = [nm for nm in ks.NAMES if not same(host(got[nm])[:d.used[nm]], R.mul[nm][:d.used[nm]])]
    assert not bad, (tag, "mul", bad)
    # mul and condensed_residual leave the solve's records alone
    assert all(same(kh.state(nm), ref) for nm, ref in (("X_REG", R.x_reg), ("Z_REG", R.z_reg), ("RHS_X_BAR", R.rxb), ("RHS_Z_BAR", R.rzb), ("LHS_Z", R.lhs_z))), (tag, "after mul")


# ---- 1. the whole shell, bitwise the oracle
@pytest.mark.parametrize("shape", ks.SHAPES, ids=str)
@pytest.mark.parametrize("sparse", EXACT)
def test_every_step_is_bitwise_the_oracle_s(hip, orc, sparse, shape):
    exits = set()
    for sh, rows, boxes, variant in ks.cases():
        if sh != shape:
            continue
        od, d, kh, ko = pair(hip, orc, *ks.problem(shape, rows, boxes, sparse), sparse, variant)
        for i, inp in enumerate(ks.step_inputs(shape, rows, boxes, sparse, variant)):
            R = reference(ko, d, inp)
            exits.add(R.exit)
            device_step(kh, d, inp, R, (shape, rows, boxes, variant, ks.STEPS[i]))
    print(shape, "loop exits met:", sorted(exits))


def test_state_is_refused_before_there_is_one(hip, orc):
    od, d, kh, ko = pair(hip, orc, *ks.problem((5, 3, 4), "mixed", "mixed", False), False, "default")
    buf = np.zeros(8)
    L = hip._lib.load()
    for what in range(5):
        assert L.pq_kktsys_state(kh.h, what, buf.ctypes.data) == PQ_ERR_INVALID and b"no factorisation" in L.pq_last_error_string()
    assert L.pq_kktsys_state(kh.h, 5, buf.ctypes.data) == PQ_ERR_INVALID and L.pq_kktsys_state(kh.h, -1, buf.ctypes.data) == PQ_ERR_INVALID
    assert L.pq_kktsys_state(None, 0, buf.ctypes.data) == PQ_ERR_INVALID and L.pq_kktsys_state(kh.h, 0, None) == PQ_ERR_INVALID
    inp = ks.step_inputs((5, 3, 4), "mixed", "mixed", False, "default")[1]
    assert kh.update_scalings_and_factor(*inp[:4])
    assert all(L.pq_kktsys_state(kh.h, what, buf.ctypes.data) == 0 for what in (0, 1))
    for what in (2, 3, 4):
        assert L.pq_kktsys_state(kh.h, what, buf.ctypes.data) == PQ_ERR_INVALID and b"no solve" in L.pq_last_error_string()
    c = kh.clone()  # a clone carries the factorisation, not the last solve
    assert L.pq_kktsys_state(c.h, 1, buf.ctypes.data) == 0 and L.pq_kktsys_state(c.h, 4, buf.ctypes.data) == PQ_ERR_INVALID
    assert kh.solve(inp[4])[0]
    assert all(L.pq_kktsys_state(kh.h, what, buf.ctypes.data) == 0 for what in range(5))


HANDFUL = [((5, 3, 4), "mixed", "mixed", "B"), ((257, 300, 64), "two-sided", "both", "D"), ((2, 7, 513), "mixed", "lower", "rate"), ((64, 257, 0), "mixed", "none", "zero-tol")]


@pytest.mark.parametrize("case", HANDFUL, ids=str)
@pytest.mark.parametrize("sparse", EXACT)
def test_device_pointers_give_the_same_bits(hip, orc, sparse, case):
    shape, rows, boxes, variant = case
    od, d, kh, ko = pair(hip, orc, *ks.problem(shape, rows, boxes, sparse), sparse, variant)
    for i, inp in enumerate(ks.step_inputs(shape, rows, boxes, sparse, variant)):
        device_step(kh, d, inp, reference(ko, d, inp), (case, ks.STEPS[i], "device" if i % 3 else "host"), torch_pointers=i % 3 != 0)  # (the pointer mode changes on a live handle too)


@pytest.mark.parametrize("case", HANDFUL, ids=str)
@pytest.mark.parametrize("sparse", EXACT)
def test_a_clone_taken_after_a_refinement_on_factorisation(hip, orc, sparse, case):
    """a clone carries the scalings, the refinement flag and the factors, and none of the work buffers: a solve on it is the solve the original would have done"""
    shape, rows, boxes, variant = case
    od, d, kh, ko = pair(hip, orc, *ks.problem(shape, rows, boxes, sparse), sparse, variant)
    steps = ks.step_inputs(shape, rows, boxes, sparse, variant)
    refine, rho, delta, v, rhs, lhs_mul = steps[3]  # the late state, refinement on
    assert refine and kh.update_scalings_and_factor(refine, rho, delta, v)
    c = kh.clone()
    R = reference(ko, d, steps[3])
    assert same(c.state("X_REG"), R.x_reg) and same(c.state("Z_REG"), R.z_reg)
    ok, lhs = c.solve(rhs)
    solve_checks(c, d, R, lhs, ok, (case, "clone: solve"))
    assert not ks.differing(d, c.mul(lhs_mul), R.mul), (case, "clone: mul")
    ok, lhs = kh.solve(rhs)
    solve_checks(kh, d, R, lhs, ok, (case, "the original after the clone's solve"))
    for i in (0, 1):  # steps of its own, refinement off then on; the original is not touched by them
        device_step(c, d, steps[i], reference(ko, d, steps[i]), (case, "clone", ks.STEPS[i]))
    assert same(kh.state("X_REG"), R.x_reg) and same(kh.state("LHS_Z"), R.lhs_z)
    device_step(kh, d, steps[5], reference(ko, d, steps[5]), (case, "the original after the clone's steps"))


@pytest.mark.parametrize("case", HANDFUL, ids=str)
@pytest.mark.parametrize("sparse", EXACT)
def test_refinement_switched_on_off_and_on_again_on_one_handle(hip, orc, sparse, case):
    """the same state and right-hand side three times: the static regularisation comes, goes and comes back, and the first and the third step agree in every bit"""
    shape, rows, boxes, variant = case
    od, d, kh, ko = pair(hip, orc, *ks.problem(shape, rows, boxes, sparse), sparse, variant)
    inp = ks.step_inputs(shape, rows, boxes, sparse, variant)[1]
    seen = []
    for refine in (1, 0, 1):
        R = reference(ko, d, (refine,) + inp[1:])
        device_step(kh, d, (refine,) + inp[1:], R, (case, "refinement", refine))
        seen.append(R)
    assert seen[0].exit >= 0 and seen[1].exit == -1 and not same(seen[0].x_reg, seen[1].x_reg)
    assert same(seen[0].x_reg, seen[2].x_reg) and not ks.differing(d, seen[0].lhs, seen[2].lhs) and seen[0].steps == seen[2].steps


# ---- 2. the shell alone, on the fast backends
def chain_problem(nx, nu, T, seed):
    P, c, A, b, G, h_l, h_u, x_l, x_u = mpc_chain(nx, nu, T, seed)
    q = dict(P=P, c=c, A=A, b=b, G=G, h_l=h_l, h_u=h_u, x_l=x_l, x_u=x_u)
    return q, np.random.default_rng(seed).uniform(0.5, 2.0, P.shape[0])


FAST = [(DENSE_CHOLESKY, False, "dense_cholesky"), (DENSE_LDLT_NO_PIVOT, False, "dense_ldlt_no_pivot"), (SPARSE_LDLT_MULTIFRONTAL, True, "sparse_ldlt_multifrontal")]
FAST_SHAPES = [((5, 3, 4), "mixed", "mixed"), ((257, 300, 64), "two-sided", "both"), ((64, 65, 63), "mixed", "none")]  # (sparse P: structurally absent diagonal entries)


def shell_only(hip, orc, q, xbs, sparse, kind, inputs, tag):
    od, d, kh, ko = pair(hip, orc, q, xbs, sparse, "B", dev_kind=kind)
    for i, inp in enumerate(inputs):
        refine, rho, delta, v, rhs, lhs_mul = inp
        R = ks.oracle_step(ko, d, *inp)
        assert R.ok_f and R.ok_s
        assert kh.update_scalings_and_factor(refine, rho, delta, v), (tag, i, "factor")
        ok, lhs = kh.solve(rhs)
        assert ok, (tag, i, "solve")
        # what does not pass through the backend is the oracle's (X_REG with refinement on also holds the backend's P_diag_device() to the oracle's diagonal)
        bad = [nm for nm, ref in (("X_REG", R.x_reg), ("Z_REG", R.z_reg), ("RHS_X_BAR", R.rxb), ("RHS_Z_BAR", R.rzb)) if not same(kh.state(nm), ref)]
        # what does is the restatement, applied to the device's own backend results
        S = ks.scalings(d, rho, delta, v)
        bad += [("recover", nm) for nm in ks.differing(d, lhs, ks.recover(d, S, rhs, lhs["x"], kh.state("LHS_Z")), ks.NAMES[2:])]
        bad += [("mul", nm) for nm in ks.differing(d, kh.mul(lhs_mul), ks.mul_from_backend(kh.backend(), d, S, lhs_mul))]
        st = kh.last_solve_stats()
        if refine:
            if not (st["backend_solves"] == st["refine_steps"] + 1 and same(st["rhs_norm"], R.rhs_norm)):
                bad.append(("stats", st))
        elif (st["refine_steps"], st["backend_solves"], st["refine_error"], st["rhs_norm"]) != (0, 1, 0.0, 0.0):
            bad.append(("stats", st))
        assert not bad, (tag, i, bad)


@pytest.mark.parametrize("shape,rows,boxes", FAST_SHAPES, ids=str)
@pytest.mark.parametrize("kind,sparse,name", FAST, ids=[f[2] for f in FAST])
def test_the_shell_around_a_fast_backend(hip, orc, kind, sparse, name, shape, rows, boxes):
    inputs = [s for s, (st, _, _) in zip(ks.step_inputs(shape, rows, boxes, sparse, "B"), ks.STEPS) if st == "early"]  # (a fast backend need not factor at the regularisation floor)
    assert [s[0] for s in inputs] == [0, 1, 0, 1]
    shell_only(hip, orc, *ks.problem(shape, rows, boxes, sparse), sparse, kind, inputs, (name, shape, rows, boxes))


@pytest.mark.parametrize("nx,nu,T", [(2, 1, 5), (3, 2, 51), (4, 2, 86)])
def test_the_shell_around_the_multistage_backend(hip, orc, nx, nu, T):
    q, xbs = chain_problem(nx, nu, T, seed=7)
    shape = (q["P"].shape[0], q["A"].shape[0], 0)
    rng = np.random.default_rng([nx, nu, T])
    inputs = []
    for refine, rk in ((0, "normal"), (1, "normal"), (0, "zero"), (1, "zero")):
        rho, delta, v = ks.state("early", shape, rng)
        inputs.append((refine, rho, delta, v, ks.rhs_of(rk, shape, rng), random_vars(*shape, rng)))
    shell_only(hip, orc, q, xbs, True, SPARSE_MULTISTAGE, inputs, ("sparse_multistage", shape))


# ---- 3. non-finite right-hand sides
@pytest.mark.parametrize("refine", [0, 1], ids=["off", "on"])
@pytest.mark.parametrize("slot", ["x", "y", "z"])
def test_a_non_finite_right_hand_side_is_seen_wherever_it_sits(hip, orc, slot, refine):
    """solve returns what the oracle's returns -- false -- for a NaN, +inf or -inf at the first and last index, and on both sides of the wave edge 64 and the block
    edge 256, of the index range no other range covers; the next solve of a clean right-hand side on the same handle succeeds and is bitwise the one before"""
    shape = ks.SLOT_SHAPES[slot]
    od, d, kh, ko = pair(hip, orc, *ks.decoupled_problem(slot), True, "default")
    rng = np.random.default_rng([ord(slot), refine])
    rho, delta, v = ks.state("early", shape, rng)
    rhs = ks.rhs_of("normal", shape, rng)
    assert ko.update_scalings_and_factor(refine, rho, delta, v) and kh.update_scalings_and_factor(refine, rho, delta, v)
    oko, ref = ko.solve(rhs)
    ok, clean = kh.solve(rhs)
    assert ok and oko and not ks.differing(d, clean, ref)
    stats = kh.last_solve_stats()
    bad = []
    for s, pos, val in ks.nonfinite_cases():
        if s != slot:
            continue
        spoiled = ks.spoiled(rhs, slot, pos, val)
        oko, _ = ko.solve(spoiled)
        ok, _ = kh.solve(spoiled)  # (what lhs holds after a failing solve is not compared)
        if ok != oko or ok:
            bad.append((pos, val, "solve returned", ok, "the oracle's", oko))
        ok, again = kh.solve(rhs)
        if not ok or ks.differing(d, again, clean) or kh.last_solve_stats() != stats:
            bad.append((pos, val, "the clean solve after it", ok, ks.differing(d, again, clean)))
    assert not bad, (slot, refine, bad)
