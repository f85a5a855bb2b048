"""CPU-only checks of tests/batch_sparse_mixed.py, the inputs of the batched sparse solver's per-instance bound sets: the lists of the forced instances are the
ones written down there, the host statement of the rules (pq_debug_bound_lists) and the CPU oracle's sparse Data agree with them and with each other on every
instance, at a setup and for the update from salt 0 to salt 1, and the oracle solves every instance of dim 16 on both backends the batch has."""
import numpy as np
import pytest

from batch_sparse_mixed import FORCED, LISTS, debug_bound_lists, forced_lists, instance_args, mixed_sparse_batch, stored_flags

B = 12


@pytest.fixture(scope="module")
def L():
    import piqp_amd
    return piqp_amd._lib.load()


def oracle_lists(od):
    return {k: od.idx(k).tolist() for k in LISTS}


@pytest.mark.parametrize("salt", [0, 1])
@pytest.mark.parametrize("dim", [16, 64])
def test_lists_of_a_setup(orc, L, dim, salt):
    bt = mixed_sparse_batch(dim, B, salt)
    n, m = dim, dim // 2
    seen = set()
    for i in range(B):
        q = instance_args(bt, i)
        od = orc.Data.sparse(**q)
        lists, dead = debug_bound_lists(L, m, n, q)
        assert lists == oracle_lists(od), i
        dropped = ~np.isfinite(q["h_l"]) & ~np.isfinite(q["h_u"])
        assert np.array_equal(dead, dropped), i
        GT = od.csc("GT")
        assert np.array_equal(dropped, [not GT.data[a:b].any() for a, b in zip(GT.indptr[:-1], GT.indptr[1:])]), (i, "the rows of G that are zeroed")
        f = (i + salt) % B
        if f in FORCED:
            seen.add(f)
            assert tuple(lists[k] for k in LISTS) == forced_lists(n, m, f), (i, f)
    assert seen == set(FORCED)


@pytest.mark.parametrize("given", [LISTS, ("h_l",), ("x_u",), ("h_l", "h_u")], ids="+".join)
@pytest.mark.parametrize("dim", [16, 64])
def test_lists_of_an_update_with_both_sides_or_boxes(orc, L, dim, given):
    """the update from salt 0 to salt 1 through the host rules, against the oracle's Solver after the same update.  With one of h_l / h_u alone the reference's
    lists can hinge on a rounding (include/piqp_amd.h at pq_solver_batch_update_dense, the second rule): those calls are held to the rule as stated instead -- the
    lists of the vectors the update leaves, a stored infinite bound being infinite."""
    b0, b1 = mixed_sparse_batch(dim, B, 0), mixed_sparse_batch(dim, B, 1)
    n, m = dim, dim // 2
    for i in range(B):
        q, q1 = instance_args(b0, i), instance_args(b1, i)
        od = orc.Data.sparse(**q)
        args = {k: q1[k] for k in given}
        lists, dead = debug_bound_lists(L, m, n, args, stored_flags(oracle_lists(od), n, m))
        if ("h_l" in given) == ("h_u" in given):
            s = orc.Solver()
            s.settings.kkt_solver = orc.SPARSE_LDLT
            assert s.setup(**q, sparse=True) and s.update(**args)
            assert lists == oracle_lists(s.data()), i
        was = ~np.isfinite(q["h_l"]) & ~np.isfinite(q["h_u"])
        keep = dict(h_l=np.where(was, -1.0, q["h_l"]), h_u=np.where(was, 1.0, q["h_u"]), x_l=q["x_l"], x_u=q["x_u"])
        eff = {k: args.get(k, keep[k]) for k in LISTS}
        assert lists == oracle_lists(orc.Data.sparse(**{**q, **eff})), i


@pytest.mark.parametrize("ks", ["SPARSE_LDLT", "SPARSE_MULTISTAGE"])
def test_the_oracle_solves_every_instance(orc, ks):
    for salt in (0, 1):
        bt = mixed_sparse_batch(16, B, salt)
        for i in range(B):
            s = orc.Solver()
            s.settings.kkt_solver = getattr(orc, ks)
            assert s.setup(**instance_args(bt, i), sparse=True)
            assert s.solve() == 1 and 3 <= s.info.iter <= 10, (salt, i, s.info.iter)
