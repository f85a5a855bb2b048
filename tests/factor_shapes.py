"""The sizes at which the dense factorisation and the triangular sweeps are held to a componentwise bound (tests/test_dense_factor_componentwise_gpu.py), each
the smallest that reaches one branch of launch_factor_panels (csrc/dense_kkt.cpp), of the ticket list of the persistent factorisation (chol_build_tasks,
csrc/dense_kernels.hip, with its defaults chol_far 2, chol_slack 3, chol_phase 1, chol_whole 22) or of launch_trsv, with the facts that prove it gets there.
tests/test_factor_plan.py re-derives every fact on the CPU (the ticket list through pq_debug_chol_plan), and checks that the size one panel smaller does NOT have
the property a shape is listed for, so a changed heuristic names the shapes that no longer reach their branch instead of the GPU test quietly testing less.

  persistent  n is a multiple of 128 and n / 128 >= 3: one persistent launch (k_chol_persistent); otherwise one fused launch per panel
  T           ceil(n / 128) panels (= tile rows)
  kind7       the largest number of multi-panel visits (task kind 7) one far tile receives: 0 below T = 9, 1 from T = 9, 2 from T = 11
  parities    the parities of the tile columns visited that way: even columns take their visits from panel 0, odd ones take the leading panel singly first
  whole       the list holds whole panel tiles (kind 2 with b == -1): rounds with >= 22 trailing tile rows, rows beyond the first two (CHOL_FAST_ROWS)
  nblk        ceil(n / 128) block rows of the sweeps; inverse = nblk >= 8: the diagonal step is one product with the double-double inverse of the 128-row block
              (below: eight steps with the inverted 16 x 16 pieces of the factorisation); H = min(7, 256 / nblk - 1) helper workgroups per block row (0 without
              the inverses).  The sweeps stay on one XCD by ticket for nblk <= 32 with H = 0, and hand over "locally" when H = 7 -- if the probe at handle creation
              found the launch dealt round robin, which Python cannot see: the GPU test therefore also runs 896, 897 and 4096 with that schedule switched off.

NOT covered: H <= 2 starts at nblk = 65 (n = 8193, a matrix of 0.5 GB and a host reference to match), and the launch-per-block-step fallback of the sweeps beyond
nblk = 224 (n > 28672).  Nothing here reaches them.

`factor` / `sweeps`: seen on an MI355X, (Cholesky, L D L^T), recorded like the LAPACK figures beside tests/assembly_shapes.py -- where the kernels stand, not a
tolerance: the bounds are derived in the test's docstring.  factor: the largest |R_ij| / (c_ij S_ij) over every factorisation of the case, i.e. as a multiple of
the bound (NumPy's and the oracle's factors reach 0.2 - 0.3 of it on the same inputs).  sweeps: the largest |r_i| / s_i of the five solves as it is; the bound c
is 9.5e-14 at n = 127 and 3.1e-12 at n = 6529.  These are far below it because s is dominated by the rank-8 part of K, which the random right-hand sides mostly
cancel; SciPy's substitution gives the same figures (1.1e-16 at 127, 3.7e-17 at 6529), and a column block left out of one block row's product is 1e-5 s.
None: the shape is not in that list."""
from collections import namedtuple

Shape = namedtuple("Shape", "n branch persistent T kind7 parities whole nblk inverse H factor sweeps")

#     n, branch, persistent, T, kind7, parities, whole, nblk, inverse, H, factor, sweeps
GRID = [
    Shape(1, "a single pivot: one short block, nothing trailing", False, 1, 0, (), False, 1, False, 0, (0.23, 0.00), None),
    Shape(16, "one 16-column piece of the diagonal block", False, 1, 0, (), False, 1, False, 0, (0.41, 0.21), None),
    Shape(17, "a second 16-column piece of one column", False, 1, 0, (), False, 1, False, 0, (0.30, 0.25), None),
    Shape(127, "a single short block, the last piece one column short", False, 1, 0, (), False, 1, False, 0, (0.39, 0.27), (1.4e-16, 9.9e-17)),
    Shape(128, "one full block, nothing trailing", False, 1, 0, (), False, 1, False, 0, (0.56, 0.31), None),
    Shape(129, "second block of one row: fuse_nb = 1, a panel of one row", False, 2, 0, (), False, 2, False, 0, (0.47, 0.32), (1.2e-16, 8.7e-17)),
    Shape(255, "second block one row short", False, 2, 0, (), False, 2, False, 0, (0.41, 0.27), None),
    Shape(256, "two full blocks, launch-per-panel (T = 2 < 3)", False, 2, 0, (), False, 2, False, 0, (0.36, 0.32), None),
    Shape(257, "third block of one row behind a full trailing tile", False, 3, 0, (), False, 3, False, 0, (0.44, 0.38), None),
    Shape(383, "T = 3 but ragged, so not persistent", False, 3, 0, (), False, 3, False, 0, (0.39, 0.30), None),
    Shape(384, "smallest persistent launch, T = 3", True, 3, 0, (), False, 3, False, 0, (0.37, 0.29), None),
    Shape(385, "T = 4 launch-per-panel with a one-row last panel", False, 4, 0, (), False, 4, False, 0, (0.32, 0.36), None),
    Shape(512, "persistent, T = 4", True, 4, 0, (), False, 4, False, 0, (0.31, 0.27), None),
    Shape(896, "nblk = 7: the last substitution form of the sweeps (persistent factorisation, T = 7)", True, 7, 0, (), False, 7, False, 0, None, (6.0e-17, 6.6e-17)),
    Shape(897, "nblk = 8: the first inverse form, a last block of one row, H = 7", False, 8, 0, (), False, 8, True, 7, None, (4.7e-17, 3.9e-17)),
    Shape(1152, "T = 9: the first multi-panel visit (kind 7: panels 0-1 on the tiles of column 8)", True, 9, 1, (0,), False, 9, True, 7, (0.50, 0.33), None),
    Shape(1408, "T = 11: visits on columns of both parities (column 9 takes panel 0 singly, then 1-2), two visits on the tiles of column 10", True, 11, 2, (0, 1),
          False, 11, True, 7, (0.50, 0.35), None),
    Shape(2944, "T = 23: the first whole panel tiles (round 0, rows beyond the first two)", True, 23, 8, (0, 1), True, 23, True, 7, (0.41, 0.27), None),
    Shape(4096, "nblk = 32: the last H = 7 and the last one-XCD size (persistent factorisation, T = 32)", True, 32, 12, (0, 1), True, 32, True, 7, None, (3.9e-17, 2.6e-17)),
    Shape(4097, "nblk = 33: H = 6", False, 33, 0, (), False, 33, True, 6, None, (4.0e-17, 4.1e-17)),
    Shape(4609, "nblk = 37: H = 5", False, 37, 0, (), False, 37, True, 5, None, (3.7e-17, 3.9e-17)),
    Shape(5377, "nblk = 43: H = 4", False, 43, 0, (), False, 43, True, 4, None, (5.3e-17, 4.8e-17)),
    Shape(6529, "nblk = 52: H = 3", False, 52, 0, (), False, 52, True, 3, None, (2.5e-17, 4.9e-17)),
]

FACTOR_SHAPES = [s for s in GRID if s.factor is not None]
SWEEP_SHAPES = [s for s in GRID if s.sweeps is not None]
# the persistent shapes that also go through update_data with a fresh P on the same handle
UPDATE_SHAPES = (384, 1408)
# (shape, PIQP_AMD_DEBUG token) of the sweep runs with a schedule switched off
SWEEP_VARIANTS = [(896, "no_one_xcd"), (897, "no_one_xcd"), (4096, "no_one_xcd"), (4096, "sweep_local=0")]
# (T, what the size one panel smaller must NOT have)
FIRST_WITH = {9: "kind7 >= 1", 11: "kind7 >= 2 with both parities", 23: "whole"}


def shape_id(s):
    return str(s.n)


def by_n(n):
    return next(s for s in GRID if s.n == n)
