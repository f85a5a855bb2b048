"""CPU-only checks of the per-instance finite-bound sets of the batched dense stack (include/piqp_amd.h): pq_debug_bound_lists, the one host function behind
pq_solver_batch_setup_dense and pq_solver_batch_update_dense, against the lists the CPU oracle holds (orc.Data.dense for a setup, orc.Solver after update() for an
update), on every instance of tests/batch_qp_mixed.py; and the refusals of pq_solver_batch_set_bound_sets, pq_kktsys_batch_create_dense_lists,
pq_kktsys_batch_set_lists and of the Python wrappers, which come before the device is touched."""
import ctypes as C

import numpy as np
import pytest

from batch_qp_mixed import hinges_on_a_rounding, mixed_batch, reference_lists_after_one_sided

PQ_OK, PQ_ERR_INVALID = 0, -1
LISTS = ("h_l", "h_u", "x_l", "x_u")
SHAPES = [(4, 2, 3, 67), (33, 0, 300, 9)]


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def ptr(a):
    return None if a is None else a.ctypes.data


def bound_lists(L, m, n, vec, fin=None):
    """pq_debug_bound_lists: vec and fin are dicts over LISTS (a missing vector is NULL; fin None is a setup).  Returns counts, lists, dead and the stored vectors,
    which start as NaN so that what the call leaves alone shows"""
    v = {k: (None if vec.get(k) is None else np.ascontiguousarray(vec[k], dtype=np.float64)) for k in LISTS}
    f = {k: (None if fin is None else np.ascontiguousarray(fin[k], dtype=np.int32)) for k in LISTS}
    counts = np.zeros(4, dtype=np.int32)
    idx = {k: np.full(max(m if k[0] == "h" else n, 1), -7, dtype=np.int32) for k in LISTS}
    dead = np.full(max(m, 1), -7, dtype=np.int32)
    out = {k: np.full(max(m if k[0] == "h" else n, 1), np.nan) for k in LISTS}
    rc = L.pq_debug_bound_lists(m, n, *[ptr(v[k]) for k in LISTS], *[ptr(f[k]) for k in LISTS], ptr(counts), *[ptr(idx[k]) for k in LISTS], ptr(dead), *[ptr(out[k]) for k in LISTS])
    assert rc == PQ_OK, L.pq_last_error_string().decode()
    lists = {k: idx[k][:c].tolist() for k, c in zip(LISTS, counts)}
    return tuple(int(c) for c in counts), lists, dead[:m], {k: a[:m if k[0] == "h" else n] for k, a in out.items()}


def flags_of(od, m, n):
    """the stored finiteness of the four vectors of an oracle's data: in the list (a dropped row is stored as -1 / 1)"""
    f = {k: np.zeros(m if k[0] == "h" else n, dtype=np.int32) for k in LISTS}
    for k in LISTS:
        f[k][od.idx(k)] = 1
    return f


def oracle_lists(od):
    return od.counts(), {k: od.idx(k).tolist() for k in LISTS}


# ---- 1. a setup
@pytest.mark.parametrize("n,p,m,batch", SHAPES, ids=str)
def test_bound_lists_of_a_setup_are_the_oracles(orc, L, n, p, m, batch):
    for i, q in enumerate(mixed_batch(n, p, m, batch)):
        od = orc.Data.dense(**q)
        counts, lists, dead, out = bound_lists(L, m, n, q)
        assert (counts, lists) == oracle_lists(od), f"instance {i}"
        dropped = ~np.isfinite(q["h_l"]) & ~np.isfinite(q["h_u"])
        assert np.array_equal(dead, dropped) and np.array_equal(dropped, ~np.array(od.mat("GT")).any(axis=0)), f"instance {i}: the dropped rows"
        for k in LISTS:  # the oracle's vectors before scaling (orc.Data.dense does not scale)
            assert np.array_equal(out[k], od.vec(k)), f"instance {i}: stored {k}"


def test_a_setup_without_vectors_has_no_bound_but_the_dropped_rows(L):
    counts, lists, dead, out = bound_lists(L, 3, 2, {})
    assert counts == (3, 3, 0, 0) and lists["h_l"] == lists["h_u"] == [0, 1, 2] and dead.all()
    assert np.array_equal(out["h_l"], [-1.0] * 3) and np.array_equal(out["h_u"], [1.0] * 3) and not out["x_l"].any() and not out["x_u"].any()


# ---- 2. an update: the stored flags of salt 0, the vectors of salt 1
def updated_oracle(orc, q, args):
    s = orc.Solver()
    assert s.setup(**q) and s.update(**args)
    return oracle_lists(s.data())  # (read while the solver lives)


def stored(q, args):
    """the four vectors after an update under the rule that a stored infinite bound is infinite: a given vector, else what the setup stored (-1 / 1 on a row it dropped)"""
    was = ~np.isfinite(q["h_l"]) & ~np.isfinite(q["h_u"])
    keep = dict(h_l=np.where(was, -1.0, q["h_l"]), h_u=np.where(was, 1.0, q["h_u"]), x_l=q["x_l"], x_u=q["x_u"])
    return {k: args.get(k, keep[k]) for k in LISTS}


@pytest.mark.parametrize("given", [LISTS, ("h_l",), ("h_u",), ("x_l",), ("x_u",), ("h_l", "x_u"), ()], ids=lambda g: "+".join(g) or "none")
@pytest.mark.parametrize("n,p,m,batch", SHAPES, ids=str)
def test_bound_lists_of_an_update_are_the_oracles(orc, L, n, p, m, batch, given):
    """Every instance against two references.  (1) orc.Solver after the same update: on every instance, but for an update of h_l or h_u alone those whose lists in
    the reference hinge on the rounding of (1e30 d) (1 / d) (hinges_on_a_rounding of tests/batch_qp_mixed.py: the library's second rule, include/piqp_amd.h); that
    such instances exist and that others remain is asserted.  On those instances, and on all others, what the reference does is asserted too: its lists are the ones
    its rules give on the stored numbers (reference_lists_after_one_sided), and where they differ from the hook's they differ on rows whose other side is stored as -/+ 1e30 and nowhere else.  (2) on EVERY instance the lists orc.Data.dense builds from the vectors the update leaves
    under that rule -- the given ones, and what the setup stored for the others."""
    changed = hinged = stray = 0
    one_sided = ("h_l" in given) != ("h_u" in given)
    for i, (q, q1) in enumerate(zip(mixed_batch(n, p, m, batch), mixed_batch(n, p, m, batch, salt=1))):
        od = orc.Data.dense(**q)
        args = {k: q1[k] for k in given}
        counts, lists, dead, out = bound_lists(L, m, n, args, flags_of(od, m, n))
        after = updated_oracle(orc, q, args)
        if one_sided:  # the predicate and the rules behind it are held to the oracle on EVERY instance: what the reference does with its stored numbers
            name = "h_l" if "h_l" in given else "h_u"
            ref = reference_lists_after_one_sided(orc, q, q1, name)[1]  # (its box lists are the setup's: a box vector given beside is not its business)
            assert all(ref[k] == after[1][k] for k in ("h_l", "h_u")), f"instance {i}: the reference's rules on its stored numbers, restated, miss the oracle"
        if one_sided and hinges_on_a_rounding(orc, q, q1, name):
            hinged += 1
            if (counts, lists) != after:
                # there the reference has left a row in neither list, or has taken a drifted row into the list of the side not given: the two differ on rows whose
                # other side is stored as -/+ 1e30 only (infinite at the setup, the row not dropped there), and nowhere else
                stray += 1
                other = "h_u" if name == "h_l" else "h_l"
                at_1e30 = set(np.flatnonzero(~np.isfinite(q[other]) & np.isfinite(q[name])).tolist())
                assert all(set(lists[k]) ^ set(after[1][k]) <= at_1e30 for k in ("h_l", "h_u")) and lists["x_l"] == after[1]["x_l"] and lists["x_u"] == after[1]["x_u"], f"instance {i}"
        else:
            assert (counts, lists) == after, f"instance {i}"
        eff = stored(q, args)
        assert (counts, lists) == oracle_lists(orc.Data.dense(**{**q, **eff})), f"instance {i}: the lists of the stored vectors"
        changed += counts != od.counts()
        # dropped in this call: both bounds infinite, a given one or the stored one (a row dropped at the setup is stored as -1 / 1); without h_l and h_u nothing
        fl, fu = np.isfinite(eff["h_l"]), np.isfinite(eff["h_u"])
        assert np.array_equal(dead, ~fl & ~fu if "h_l" in given or "h_u" in given else np.zeros(m, dtype=bool)), f"instance {i}: the dropped rows"
        for k in LISTS:
            if k[0] == "x":  # a given box vector is packed to its new list, one that is not given is not touched
                exp = np.concatenate([q1[k][lists[k]], np.zeros(n - len(lists[k]))]) if k in given else np.full(n, np.nan)
                assert np.array_equal(out[k], exp, equal_nan=True), f"instance {i}: stored {k}"
            else:  # a given row vector at full length; the other side on the rows dropped in this call only
                sign = -1.0 if k == "h_l" else 1.0
                exp = np.where(dead != 0, sign, np.where(np.isfinite(q1[k]), q1[k], sign * 1e30)) if k in given else np.where(dead != 0, sign, np.nan)
                assert np.array_equal(out[k], exp, equal_nan=True), f"instance {i}: stored {k}"
    if one_sided:
        # (4, 2, 3, 67): 6 resp. 5 of 67 for h_l / h_u alone; (33, 0, 300, 9), where a row of 300 drifts in most instances: 5 resp. 5 of 9
        assert 0 < hinged < batch, (hinged, "instances whose reference lists hinge on a rounding: some, and not all")
        assert 0 < stray <= hinged, (stray, "of them, instances in which the rounding went against the library's rule: where the product came back to 1e30 the two agree")
    if given == LISTS:
        assert changed >= batch - 2, "the update is to change the sets"


def test_minus_infinity_on_a_dropped_row_keeps_the_row_when_h_u_is_absent(orc, L):
    n, p, m, batch = 4, 2, 3, 67
    q = mixed_batch(n, p, m, batch)[3]  # every row dropped: stored as -1 / 1
    od = orc.Data.dense(**q)
    assert od.counts()[:2] == (m, m)
    args = dict(h_l=np.full(m, -np.inf))
    counts, lists, dead, out = bound_lists(L, m, n, args, flags_of(od, m, n))
    assert (counts, lists) == updated_oracle(orc, q, args)
    assert counts[:2] == (0, m) and not dead.any(), "the stored 1 keeps the row: it is not dropped again"
    assert np.array_equal(out["h_l"], [-1e30] * m) and np.isnan(out["h_u"]).all()


# ---- 3. refusals before the device is touched
def test_bound_sets_mode_and_null_handle(L):
    h = C.c_void_p()
    assert L.pq_solver_batch_create(C.byref(h), 0) == PQ_OK
    for bad in (2, -1, 7):
        assert L.pq_solver_batch_set_bound_sets(h, bad) == PQ_ERR_INVALID and L.pq_last_error_string().decode()
    assert L.pq_solver_batch_set_bound_sets(h, 1) == PQ_OK and L.pq_solver_batch_set_bound_sets(h, 0) == PQ_OK
    assert L.pq_solver_batch_set_bound_sets(None, 1) == PQ_ERR_INVALID and L.pq_last_error_string().decode()
    L.pq_solver_batch_destroy(h)
    assert L.pq_kktsys_batch_set_lists(None, None, None, None, None, None) == PQ_ERR_INVALID and L.pq_last_error_string().decode()


def create_lists(L, batch, n, p, m, counts, lists):
    import piqp_amd
    h = C.c_void_p()
    P, A, G = np.zeros((batch, n, n)), np.zeros((batch, p, n)), np.zeros((batch, m, n))
    st = piqp_amd.default_settings()
    rc = L.pq_kktsys_batch_create_dense_lists(C.byref(h), 0, batch, n, p, m, ptr(P), ptr(A), ptr(G), ptr(counts), *[ptr(l) for l in lists], None, C.byref(st), 0)
    assert not h.value
    return rc, L.pq_last_error_string().decode()


def test_the_per_instance_creator_refuses_bad_lists_and_names_the_instance(L):
    batch, n, p, m = 5, 4, 1, 3

    def good():
        counts = np.tile(np.array([m, m, 2, 1], dtype=np.int32), (batch, 1))
        lists = [np.tile(np.arange(m, dtype=np.int32), (batch, 1)), np.tile(np.arange(m, dtype=np.int32), (batch, 1)), np.tile(np.array([0, 2, 0, 0], dtype=np.int32), (batch, 1)),
                 np.tile(np.array([3, 0, 0, 0], dtype=np.int32), (batch, 1))]
        return counts, lists

    counts, lists = good()
    rc, text = create_lists(L, batch, n, p, m, None, lists)
    assert rc == PQ_ERR_INVALID and "counts" in text
    counts, lists = good()
    counts[1, 2] = n + 1  # a count above its length
    rc, text = create_lists(L, batch, n, p, m, counts, lists)
    assert rc == PQ_ERR_INVALID and "instance 1" in text and "n_x_l" in text
    counts, lists = good()
    lists[2][2, :2] = (2, 0)  # not ascending in instance 2 only
    rc, text = create_lists(L, batch, n, p, m, counts, lists)
    assert rc == PQ_ERR_INVALID and "instance 2" in text and "ascending" in text
    counts, lists = good()
    counts[batch - 1, :2] = (2, 1)  # the last instance: rows 0, 1 in h_l_idx, row 0 in h_u_idx, row 2 in neither
    rc, text = create_lists(L, batch, n, p, m, counts, lists)
    assert rc == PQ_ERR_INVALID and f"instance {batch - 1}" in text and "row 2" in text and "neither" in text
    counts, lists = good()
    lists[3][0, 0] = n  # out of range
    rc, text = create_lists(L, batch, n, p, m, counts, lists)
    assert rc == PQ_ERR_INVALID and "instance 0" in text and "outside" in text


def test_the_python_wrappers_refuse_before_any_library_call():
    import piqp_amd
    for bad in ("x", "", "SHARED", None):
        with pytest.raises(ValueError, match="bounds"):
            piqp_amd.BatchDenseSolver(bounds=bad)
    assert piqp_amd.BatchDenseSolver().bounds == "shared" and piqp_amd.BatchDenseSolver(bounds="per_instance").bounds == "per_instance"
    batch, n, p, m = 3, 4, 0, 2
    P, G = np.zeros((batch, n, n)), np.zeros((batch, m, n))
    one = ([0, 1], [0], [1, 3], [])
    make = lambda lists: piqp_amd.BatchKKTSystem.per_instance(P, None, G, lists)
    for lists, err in (([one, one], ValueError), ([one, one, one[:3]], ValueError), (5, TypeError), ([one, one, ([0], [0], [], [])], ValueError),
                       ([one, one, ([0, 1], [0], [3, 1], [])], ValueError), ([one, one, ([0, 1], [0], [1, 4], [])], ValueError), ([one, one, ([0, 1], [0], [0.5], [])], TypeError),
                       ([one, one, ([0, 1, 1], [0], [], [])], ValueError)):
        with pytest.raises(err):
            make(lists)
