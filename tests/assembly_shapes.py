"""The shapes at which the dense KKT assembly is held to a NumPy reference (tests/test_dense_assembly_gpu.py), each the smallest that reaches one branch of
launch_syrk (csrc/dense_kernels.hip), with the launch plan that branch needs: what pq_debug_syrk_plan answers for 256 CUs (512 workgroup slots).

A plan is (T, ntiles, low_latency, tile_order, rem, k_split):
  T           = ceil(n / 128) tile rows, ntiles = T (T + 1) / 2 tiles of the lower triangle
  low_latency = kdim <= 256: the main launch is <EPI, 4, 4> with 1024 threads, otherwise <EPI, 2, 2> with 256
  tile_order  = T >= 16 and not low_latency: the XCD-aware order table (8 x 8 patches dealt to 8 XCDs) replaces the triangular block -> tile map
  rem, k_split: the last `rem` tiles run as k_split K-slices each (<EPI, 2, 2>, raw partial tiles) + k_syrk_tail_reduce; (0, 1) = no tail

`assembly` is the plan of the G' W G launch (kdim = m, with the split workspace; None for m = 0, where k_assemble_no_g runs instead), `ata` the plan of the
A^T A launch of upload() (kdim = p, EPI_STORE, never split; None for p = 0).  tests/test_syrk_plan.py re-derives every tuple on the CPU and compares it with the
library's answer, so a changed heuristic names the shapes that no longer reach their branch instead of the GPU test quietly testing less."""
from collections import namedtuple

Shape = namedtuple("Shape", "n p m assembly ata branch")

GRID = [
    Shape(513, 0, 17, (5, 15, 1, 0, 0, 1), None,
          "one-row ragged tile row, odd lda (scalar loads), K = one full stage + a stage of one column, 16-wave shape"),
    Shape(514, 0, 300, (5, 15, 0, 0, 0, 1), None,
          "aligned interior fast path beside checked edge tiles (two ragged rows); kdim = 18 * 16 + 12, 4-wave shape"),
    Shape(640, 0, 256, (5, 15, 1, 0, 0, 1), None, "the last kdim of the 16-wave shape"),
    Shape(640, 0, 257, (5, 15, 0, 0, 0, 1), None, "the first kdim of the 4-wave shape; the final K stage holds one column"),
    Shape(384, 300, 0, None, (3, 6, 0, 0, 0, 1), "<EPI_STORE, 2, 2> into ATA (p > 256), then k_assemble_no_g with ATA"),
    Shape(1000, 257, 40, (8, 36, 1, 0, 0, 1), (8, 36, 0, 0, 0, 1),
          "big-K ATA (4-wave EPI_STORE) added in the EPI_ASSEMBLE epilogue of the 16-wave shape, ragged last tile row (104 rows)"),
    Shape(1920, 0, 272, (15, 120, 0, 0, 0, 1), None, "T = 15: the largest grid without the tile-order table"),
    Shape(1921, 0, 272, (16, 136, 0, 1, 0, 1), None, "T = 16: table on, one-row ragged tile row, odd lda"),
    Shape(1922, 130, 272, (16, 136, 0, 1, 0, 1), (16, 136, 1, 0, 0, 1),
          "T = 16, aligned, two-row ragged tile row, ATA from the 16-wave shape (no table: kdim = 130)"),
    Shape(2176, 0, 272, (17, 153, 0, 1, 0, 1), None, "T = 17: full tiles, partial 8 x 8 patches, 153 = 8 * 19 + 1 tiles in uneven XCD chunks"),
    Shape(4096, 0, 128, (32, 528, 1, 0, 16, 2), None, "tail of 16 tiles behind a 16-wave main launch, 4-wave tail, 8 K stages in 2 slices of 4"),
    Shape(4100, 0, 200, (33, 561, 1, 0, 49, 3), None,
          "T = 33: ragged tiles (4 rows) inside a tail of 49 tiles, 13 K stages in slices of 5 / 5 / 3, the last stage 8 columns"),
    Shape(4100, 0, 520, (33, 561, 0, 1, 49, 8), None,
          "k_split = 8 over 33 K stages: kt_per = 5, slice 6 = stages 30..32 ending in an 8-column stage, slice 7 empty; table on, T = 33"),
]

# the shapes whose factorisation and solve are checked too (both kkt_solver 0 and 16): (1921, 0, 272) and (4100, 0, 200) factor launch-per-panel (n is no multiple of
# 128) at T = 16 and T = 33 with a ragged last panel, and the sweeps of n = 4100 (33 block rows) leave the one-XCD schedule
# These matrices are well conditioned by construction: numpy.linalg.solve (LAPACK, fp64) on the reference matrix E meets the residual expression of
# tests/test_dense_assembly_gpu.py::test_factor_and_solve_residual with |E x - b|_inf / |b|_inf =
#   (1921, 0, 272): 7.6e-15   (4100, 0, 200): 1.2e-14   (1000, 257, 40): 4.0e-15   (2176, 0, 272): 8.1e-15
# so the 1e-10 bar has four orders of magnitude to spare and tests the device (test_solve_shapes_are_well_conditioned asserts a factor 10 on the CPU)
SOLVE_SHAPES = [(1921, 0, 272), (4100, 0, 200), (1000, 257, 40), (2176, 0, 272)]
# ... and those that also go through update_data with fresh P, A, G on the same handle
UPDATE_SHAPES = [(514, 0, 300), (1922, 130, 272), (4100, 0, 520)]


def shape_id(s):
    return f"{s.n}-{s.p}-{s.m}"


def by_dims(dims):
    return next(s for s in GRID if (s.n, s.p, s.m) == tuple(dims))
