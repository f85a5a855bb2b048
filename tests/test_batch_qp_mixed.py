"""tests/batch_qp_mixed.py on the CPU oracle alone: at the shapes the GPU tests of the per-instance bound sets use, with both factorisations, every instance of
mixed_batch ends SOLVED, the instances of a batch do not run in lock step, they hold at least three different sets of counts, and the four forced patterns are
there with the lists DenseSolver holds for them."""
import numpy as np
import pytest

from batch_qp_mixed import forced_lists, mixed_batch, oracle_of_mixed

LLT, LDLT = 0, 16
SOLVED = 1
SHAPES = [(1, 0, 0, 9), (4, 2, 3, 67), (33, 0, 300, 9), (32, 3, 5, 9), (128, 7, 5, 9)]
LISTS = ("h_l", "h_u", "x_l", "x_u")


@pytest.mark.parametrize("kind", [LLT, LDLT], ids=["llt", "ldlt"])
@pytest.mark.parametrize("n,p,m,batch", SHAPES, ids=str)
def test_mixed_batch_on_the_oracle(orc, n, p, m, batch, kind):
    import piqp_amd
    qs, ref = oracle_of_mixed(orc, piqp_amd, n, p, m, batch, kind)
    assert all(o["status"] == SOLVED for o in ref), [o["status"] for o in ref]
    assert len({o["info"]["iter"] for o in ref}) >= 2, "the instances must not run in lock step"
    data = [orc.Data.dense(**q) for q in qs]
    assert len({d.counts() for d in data}) >= 3, "the instances must hold different sets of finite bounds"
    for f in range(4):
        assert [data[f].idx(k).tolist() for k in LISTS] == [list(l) for l in forced_lists(n, m, f)], f"forced pattern {f}"
    if m:
        assert not np.array(data[3].mat("GT")).any() and (data[3].vec("h_l") == -1).all() and (data[3].vec("h_u") == 1).all(), "instance 3: every row dropped"


@pytest.mark.parametrize("n,p,m,batch", [(4, 2, 3, 67), (33, 0, 300, 9)], ids=str)
def test_salt_changes_the_patterns_only(orc, n, p, m, batch):
    a, b = mixed_batch(n, p, m, batch, 0), mixed_batch(n, p, m, batch, 1)
    changed = 0
    for qa, qb in zip(a, b):
        assert all(np.array_equal(qa[k], qb[k]) for k in ("P", "c", "G") if k in qa)
        for k in ("h_l", "h_u", "x_l", "x_u"):
            both = np.isfinite(qa[k]) & np.isfinite(qb[k])
            assert np.array_equal(qa[k][both], qb[k][both]), "a bound that is finite under both salts is the same number"
        changed += orc.Data.dense(**qa).counts() != orc.Data.dense(**qb).counts()
    assert changed >= batch - 2
