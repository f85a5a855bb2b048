"""Worker of tests/test_batch_sparse_clone_gpu.py::test_arena_gather_in_both_word_widths: clones of solved batches by a permutation and by a fan-out list, compared
with their sources bit for bit, before and after an update on both.  PIQP_AMD_DEBUG of the parent selects the word width of the arena gather (the library parses it
once per process) and makes the library report the width it took on stderr."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import piqp_amd as hip  # noqa: E402
from batch_sparse_mixed import sub_batch  # noqa: E402
from test_batch_bounds_gpu import _assert_same, _handle, _moved, _mpc_as_batch, _solved, _vectors  # noqa: E402
from test_batch_ldlt_gpu import _random_sparse_qp_batch  # noqa: E402

B = 12
PERM = [5, 0, 11, 3, 8, 1, 10, 2, 7, 4, 9, 6]
for ks, bt in ((hip.SPARSE_MULTISTAGE, _mpc_as_batch(B)), (hip.SPARSE_MULTISTAGE, _random_sparse_qp_batch(16, B, seed=16)), (hip.SPARSE_LDLT, _random_sparse_qp_batch(16, B, seed=16))):
    src = _handle(hip, bt, ks, "shared")
    ref = _solved(src)
    b1 = _moved(bt, 1)
    clones = [(idx, src.clone(idx)) for idx in (PERM, [0] * 20)]
    for idx, cl in clones:
        for k in ("x", "y", "z_l", "z_u", "z_bl", "z_bu", "s_l", "s_u", "s_bl", "s_bu"):
            assert np.array_equal(cl.result(k), ref[k][idx]), k
        _assert_same(_solved(cl), ref, None, idx, what="clone")
        assert cl.update_data(P_values=b1["Pv"][idx], **_vectors(sub_batch(b1, idx)))
    assert src.update_data(P_values=b1["Pv"], **_vectors(b1))
    ref = _solved(src)
    for idx, cl in clones:
        _assert_same(_solved(cl), ref, None, idx, what="update_data")
