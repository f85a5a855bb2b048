/*
 * piqp_amd.h -- C-ABI of the MI355X-native KKT backend for PIQP (libpiqp_amd.so).
 *
 * Drop-in boundary: these entry points are what a PIQP build would bind to replace the bodies of its
 * KKT plugin interface and of the KKTSystem shell that drives it.  Every function cites the reference
 * interface it replaces (paths relative to PIQP v0.6.2 include/piqp/).  INTEGRATION.md shows the
 * reference-side adapter class (a KKTSolverBase<T,I,PIQP_DENSE> subclass calling pq_kkt_*).
 *
 * Conventions
 *   - fp64 everywhere, column-major dense matrices, int32 index lists (common.hpp:38-39, typedefs.hpp:53-68).
 *   - Opaque handles own all device memory; nothing is allocated after *_create (the reference's tests
 *     enforce alloc-free factor/solve: fwd.hpp:44-52).
 *   - Return: >= 0 success (factor calls: 1 = factorised, 0 = numerical failure exactly where the
 *     reference returns false), < 0 = pq_status error.  Nothing throws across this boundary.
 *   - Vector arguments live where the handle's pointer mode says: PQ_MEM_HOST (default; the library
 *     stages them through its own pinned buffers -- this is the reference's calling convention) or
 *     PQ_MEM_DEVICE (already resident in HBM; no copies, calls are asynchronous on the handle's stream
 *     except where a scalar must come back to the host).
 *   - A handle is not thread-safe; distinct handles may be used concurrently (one HIP stream each),
 *     like independent solver copies in the reference (kkt_system.hpp:70-95).
 *   - There is no CPU fallback: if no HIP device is usable, *_create fails with PQ_ERR_HIP.
 */
#ifndef PIQP_AMD_H
#define PIQP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PQ_OK = 0,
    PQ_ERR_INVALID = -1,     /* bad argument / size mismatch */
    PQ_ERR_HIP = -2,         /* HIP runtime error (see pq_last_error_string) */
    PQ_ERR_UNSUPPORTED = -3, /* kkt solver not supported (kkt_system.hpp:464-465,493-494) */
    PQ_ERR_NOMEM = -4,
    PQ_ERR_INTERNAL = -5     /* a bounded loop of the library reached its bound (pq_solver_batch_solve) */
} pq_status;

typedef enum { PQ_MEM_HOST = 0, PQ_MEM_DEVICE = 1 } pq_mem;

/* settings.hpp:18-26 KKTSolver (+ the in-tree pivot-free LDLt of dense/ldlt_no_pivot.hpp as a second dense kernel) */
typedef enum {
    PQ_DENSE_CHOLESKY = 0,
    PQ_SPARSE_LDLT = 1,
    PQ_SPARSE_LDLT_EQ_COND = 2,
    PQ_SPARSE_LDLT_INEQ_COND = 3,
    PQ_SPARSE_LDLT_COND = 4,
    PQ_SPARSE_MULTISTAGE = 5,
    PQ_DENSE_LDLT_NO_PIVOT = 16,
    /* the two engines behind PQ_SPARSE_LDLT, selectable directly (not in the reference's enum): the reference's own up-looking elimination order on the
     * device (sparse/ldlt.hpp:101-218 bit for bit; PQ_SPARSE_LDLT picks it up to 8192 KKT rows and 4e7 flops per factorisation -- 3e9 in the condensed modes) and the
     * supernodal multifrontal LDLt (everything else) */
    PQ_SPARSE_LDLT_EXACT = 17,
    PQ_SPARSE_LDLT_MULTIFRONTAL = 18,
    /* the dense Cholesky backend in the reference's own order of floating-point operations (csrc/dense_exact.hip): assembly, factor, solves and mat-vecs bitwise
     * the CPU oracle's, whole solves with its iteration counts.  n <= 1024 (PQ_ERR_UNSUPPORTED above); never chosen by default -- the yardstick for
     * PQ_DENSE_CHOLESKY, as PQ_SPARSE_LDLT_EXACT is for the sparse engines */
    PQ_DENSE_CHOLESKY_EXACT = 19
} pq_kkt_solver;

/* kkt_fwd.hpp:23-29 KKTUpdateOptions */
enum { PQ_KKT_UPDATE_NONE = 0, PQ_KKT_UPDATE_P = 1, PQ_KKT_UPDATE_A = 2, PQ_KKT_UPDATE_G = 4 };

/* results.hpp:18-27 Status */
enum {
    PQ_SOLVED = 1,
    PQ_MAX_ITER_REACHED = -1,
    PQ_PRIMAL_INFEASIBLE = -2,
    PQ_DUAL_INFEASIBLE = -3,
    PQ_NUMERICS = -8,
    PQ_UNSOLVED = -9,
    PQ_INVALID_SETTINGS = -10
};

/* dense/data.hpp:22-51 -- the (Ruiz-scaled) problem data a backend reads.  Matrices are the TRANSPOSED
 * constraint matrices exactly as dense::Data stores them.  `mem` says where these arrays live. */
typedef struct {
    int n, p, m;
    const double *P_utri; /* n x n, upper triangle read */
    const double *AT;     /* n x p */
    const double *GT;     /* n x m */
    /* the remaining fields are only read by pq_kktsys_* (KKTSystem), never by pq_kkt_* (backend) */
    int n_h_l, n_h_u, n_x_l, n_x_u;
    const int *h_l_idx, *h_u_idx, *x_l_idx, *x_u_idx; /* finite-bound index lists, ascending */
    const double *x_b_scaling;                         /* n, NULL = all ones */
    int mem;                                           /* pq_mem */
} pq_dense_data;

/* sparse/data.hpp:26-54 -- CSC int32/fp64 (P_utri upper triangle; AT = A^T n x p; GT = G^T n x m).
 * Every index array (*_colptr, *_rowind, *_idx) is HOST memory in either mode: the symbolic analysis runs on the host.  `mem` says where the value arrays P_val,
 * AT_val, GT_val and x_b_scaling live: PQ_MEM_HOST, or PQ_MEM_DEVICE = device memory on the handle's device (complete before the call, only read, read by the time
 * the call returns).  Device mode, every sparse backend (PQ_SPARSE_LDLT on either engine, the condensed modes, PQ_SPARSE_MULTISTAGE, selectors 17 and 18): *_create
 * and *_update_data_sparse move the values device-to-device, nothing crosses the host-device link and no value is ever fetched to the host (a handle that has to
 * remember its data for pq_kkt_partition keeps a device copy).  Any other value of mem: PQ_ERR_INVALID, the handle stays as it was. */
typedef struct {
    int n, p, m;
    const int *P_colptr, *P_rowind; const double *P_val;
    const int *AT_colptr, *AT_rowind; const double *AT_val;
    const int *GT_colptr, *GT_rowind; const double *GT_val;
    int n_h_l, n_h_u, n_x_l, n_x_u;
    const int *h_l_idx, *h_u_idx, *x_l_idx, *x_u_idx;
    const double *x_b_scaling;
    int mem; /* pq_mem: where the VALUE arrays live; the index arrays are host memory always */
} pq_sparse_data;

/* variables.hpp:19-105 Variables<T>: ten vectors (box vectors length n, compressed to the first
 * n_x_l / n_x_u entries exactly as the reference keeps them) */
typedef struct {
    double *x, *y, *z_l, *z_u, *z_bl, *z_bu, *s_l, *s_u, *s_bl, *s_bu;
} pq_vars;

/* settings.hpp:43-82 Settings<T> (same fields, same defaults via pq_settings_default) */
typedef struct {
    double rho_init, delta_init;
    double eps_abs, eps_rel;
    int check_duality_gap;
    double eps_duality_gap_abs, eps_duality_gap_rel;
    double infeasibility_threshold;
    double reg_lower_limit, reg_finetune_lower_limit;
    int reg_finetune_primal_update_threshold, reg_finetune_dual_update_threshold;
    int max_iter, max_factor_retires;
    int preconditioner_scale_cost, preconditioner_reuse_on_update, preconditioner_iter;
    double tau;
    int kkt_solver; /* pq_kkt_solver */
    int iterative_refinement_always_enabled;
    double iterative_refinement_eps_abs, iterative_refinement_eps_rel;
    int iterative_refinement_max_iter;
    double iterative_refinement_min_improvement_rate;
    double iterative_refinement_static_regularization_eps;
    double iterative_refinement_static_regularization_rel;
    int verbose, compute_timings;
} pq_settings;

/* results.hpp:45-89 Info<T> */
typedef struct {
    int status;
    int iter;
    double rho, delta, mu, sigma, primal_step, dual_step;
    double primal_res, primal_res_rel, dual_res, dual_res_rel;
    double primal_res_reg, primal_res_reg_rel, dual_res_reg, dual_res_reg_rel;
    double primal_prox_inf, dual_prox_inf;
    double prev_primal_res, prev_dual_res;
    double primal_obj, dual_obj, duality_gap, duality_gap_rel;
    int factor_retires;
    double reg_limit;
    int no_primal_update, no_dual_update;
    double setup_time, update_time, solve_time, kkt_factor_time, kkt_solve_time, run_time;
    int n_factor, n_solve, n_backend_solve; /* call counters (not in the reference) */
} pq_info;

void pq_settings_default(pq_settings *s);       /* settings.hpp:45-82 */
const char *pq_last_error_string(void);          /* thread-local text of the last < 0 return */
int pq_device_count(void);                       /* number of visible HIP devices (0 = library unusable) */
const char *pq_version(void);

/* ===================== KKT backend: replaces KKTSolverBase<T,I,MatrixType> ===================== */
typedef struct pq_kkt pq_kkt;

/* dense::KKT ctor, dense/kkt.hpp:39-55 (uploads P_utri/AT/GT, builds AT_A = AT*AT^T).
 * kkt_solver: PQ_DENSE_CHOLESKY (Eigen::LLT semantics, dense/kkt.hpp:82-83), PQ_DENSE_LDLT_NO_PIVOT or PQ_DENSE_CHOLESKY_EXACT (n <= 1024). */
int pq_kkt_create_dense(pq_kkt **out, const pq_dense_data *data, int kkt_solver, int device);
/* sparse::KKT ctor, sparse/kkt.hpp:51-70 (assemble KKT by mode, AMD, permute, symbolic, upload) for
 * kkt_solver = PQ_SPARSE_LDLT; MultistageKKT ctor, sparse/multistage_kkt.hpp:76-135 (arrow-structure
 * detection, block containers, AtA) for kkt_solver = PQ_SPARSE_MULTISTAGE */
int pq_kkt_create_sparse(pq_kkt **out, const pq_sparse_data *data, int kkt_solver, int device);
int pq_kkt_clone(const pq_kkt *k, pq_kkt **out); /* kkt_solver_base.hpp:28 clone() */
void pq_kkt_destroy(pq_kkt *k);                  /* kkt_solver_base.hpp:26 */
int pq_kkt_set_pointer_mode(pq_kkt *k, int mem); /* where vector arguments of the calls below live */
/* kkt_solver_base.hpp:30 update_data(data, options): re-reads the flagged matrices from `data`
 * (dense re-uploads all three on every call, see SURVEY.md section 7 last bullet) */
int pq_kkt_update_data_dense(pq_kkt *k, const pq_dense_data *data, int options);
int pq_kkt_update_data_sparse(pq_kkt *k, const pq_sparse_data *data, int options);
/* kkt_solver_base.hpp:32: returns 1 ok / 0 failed.  dense: llt.info()==Success (dense/kkt.hpp:83);
 * sparse: n == cols (sparse/kkt.hpp:104).  x_reg[n], z_reg[m] are consumed during the call. */
int pq_kkt_update_scalings_and_factor(pq_kkt *k, double delta, const double *x_reg, const double *z_reg);
/* kkt_solver_base.hpp:34 solve(): outputs caller-allocated (n, p, m) */
int pq_kkt_solve(pq_kkt *k, const double *rhs_x, const double *rhs_y, const double *rhs_z, double *lhs_x,
                 double *lhs_y, double *lhs_z);
/* kkt_solver_base.hpp:37 z = alpha * P * x */
int pq_kkt_eval_P_x(pq_kkt *k, double alpha, const double *x, double *z);
/* kkt_solver_base.hpp:39 zn = alpha_n * A * xn, zt = alpha_t * A^T * xt */
int pq_kkt_eval_A_xn_and_AT_xt(pq_kkt *k, double alpha_n, double alpha_t, const double *xn, const double *xt,
                               double *zn, double *zt);
/* kkt_solver_base.hpp:41 zn = alpha_n * G * xn, zt = alpha_t * G^T * xt */
int pq_kkt_eval_G_xn_and_GT_xt(pq_kkt *k, double alpha_n, double alpha_t, const double *xn, const double *xt,
                               double *zn, double *zt);
int pq_kkt_print_info(pq_kkt *k);                                   /* kkt_solver_base.hpp:43 */
int pq_kkt_synchronize(pq_kkt *k);                                  /* wait for the handle's stream (everything a later call of the handle depends on is ordered behind it on the device) */
void *pq_kkt_stream(pq_kkt *k);                                     /* hipStream_t of the handle */
/* test hooks: dense/kkt.hpp:134 internal_kkt_mat() and the factor; copy n*n doubles to HOST memory */
int pq_kkt_internal_kkt_mat(pq_kkt *k, double *out_host);
int pq_kkt_internal_factor(pq_kkt *k, double *out_host);
int pq_kkt_dims(const pq_kkt *k, int *n, int *p, int *m);
/* sparse_multistage only: what MultistageKKT::print_info reports (multistage_kkt.hpp:385-393).  Writes up to
 * `capacity` rows of (start, diag_size, off_diag_size) -- the last row is the arrow corner block -- and
 * returns the number of blocks (call with out_host = NULL to size the buffer). */
int pq_kkt_multistage_block_info(pq_kkt *k, int *out_host, int capacity);
/* sparse_multistage only (an error for every other backend), read-only: where the chain kernels keep their working set, decided from the block
 * structure at setup.  out = { engine (0 chain, 1 tree), factor_in_lds, li_in_lds, solve_in_lds, asm_chunks, max_h, max_w, factor_lds_bytes }:
 * the frontal matrix factored in LDS or in place in HBM, the inverse of the diagonal block staged in LDS or written straight to HBM, the
 * substitution's panel in LDS or read from HBM, workgroups per stage of the assembly, largest front order, largest panel width, dynamic LDS
 * of the factorisation kernel. */
int pq_kkt_multistage_plan(pq_kkt *k, int out[8]);
/* sparse backends: figures of the symbolic analysis for roofline arithmetic.  out = { N, nnz(PKPt), nnz(L) below
 * the diagonal, supernodes, tree levels, workgroup subtrees, max front order, factorisation flops sum_j (c_j^2 + 3 c_j) } */
int pq_kkt_sparse_stats(pq_kkt *k, double out[8]);
/* ---- stage-partitioned execution of ONE KKT system over several processes, one GPU each (BASELINE configs[4]; the
 * reference has no counterpart, its multistage backend is a serial recurrence, multistage_kkt.hpp:1289-1347,1726-1814).
 * Every process creates the same backend on the same data and calls pq_kkt_partition with its rank.  Vectors stay
 * replicated; the assembly-tree work of factor / solve is split: each rank eliminates the subtrees it owns (for a
 * multistage chain: a contiguous range of stages), the update matrices of the subtree roots are summed across ranks,
 * and the few supernodes above them are eliminated by every rank on identical data.  The library never talks to the
 * network itself: when data has to cross ranks it synchronises its stream and calls `exchange(user, which)`, and the
 * caller performs the collective on the buffer it registered (torch.distributed over RCCL in piqp_amd/dist.py):
 *   which = 0  all-reduce(sum) of buf_factor [sizes[0] doubles]   once per factorisation
 *   which = 1  all-reduce(sum) of buf_forward [sizes[1] doubles]  once per backend solve
 *   which = 2  all-gather in place of buf_gather [world x sizes[2] doubles, this rank's chunk at rank * sizes[2]]
 * The callback returns 0 on success; it must return only when the result is visible to the handle's stream.
 * Supported by the sparse_ldlt* backends and by sparse_multistage when it runs on the tree engine. */
typedef int (*pq_exchange_fn)(void *user, int which);
int pq_kkt_partition(pq_kkt *k, int rank, int world, long long sizes_out[3]);
int pq_kkt_set_exchange(pq_kkt *k, pq_exchange_fn exchange, void *user, double *buf_factor, double *buf_forward,
                        double *buf_gather);
/* Native transport (the north star's "RCCL over xGMI"): instead of a callback the library creates its own communicator and enqueues the three
 * collectives -- ncclAllReduce(sum, fp64) for which = 0, 1 and ncclAllGather for which = 2 -- on the handle's stream, right behind the kernels that
 * pack its own exchange buffers: no stream drain, no host round trip.  Rank 0 obtains the 128-byte id (pq_rccl_unique_id = ncclGetUniqueId) and
 * ships it to the other ranks by any means (MPI_Bcast, a file, torch.distributed.broadcast_object_list in piqp_amd/dist.py); then EVERY rank calls
 * pq_kkt_set_comm_rccl after pq_kkt_partition with the rank / world it partitioned with (collective: ncclCommInitRank).  One process per GPU.
 * librccl is loaded with dlopen at the first of these calls; single-GPU use never needs it. */
int pq_rccl_unique_id(unsigned char id_out[128]);
int pq_kkt_set_comm_rccl(pq_kkt *k, const unsigned char id[128], int rank, int world);
/* SURVEY 8(e) row 2 (reference: the stage-parallel loops of sparse/multistage_kkt.hpp:856-993, 1036-1218, 1529-1643): with a stage partition of a sparse_ldlt
 * (KKT_FULL) backend, (a) the per-factorisation value assembly refreshes only the diagonal entries of the fronts this rank factors, and (b) the refinement
 * residual err = rhs - K lhs (kkt_system.hpp:507-536) is evaluated only on the rows this rank's part of the next solve reads; ||err||_inf crosses the ranks in
 * ONE collective per refinement step:
 *   which = 3  all-reduce(MAX) of buf_norm [1 double]
 * through the same callback (register buf_norm after pq_kkt_set_exchange) or, with the native transport, ncclAllReduce(max) on the library's own buffer.  No halo
 * exchange is needed: the solution vectors are replicated (which = 2 gathers them), so every rank reads what its rows touch.  Without a registered buffer, for the
 * condensed KKT modes, or with PIQP_AMD_DEBUG=replicated_residual the residual is evaluated on every row by every rank as before.  The results are bitwise those of
 * the replicated evaluation (tests/test_partition.py).  pq_kkt_sharded_calls: out[0] = sharded residual evaluations so far, out[1] = rows in this rank's share.
 * Condensed KKT modes and sparse_multistage (tree engine): a partitioned handle re-evaluates, per factorisation, only the values of the fronts it factors (P entries,
 * delta^-1 A^T A entries, G^T W G product terms, diagonal shifts selected by destination front); there pq_kkt_sharded_calls reports out[0] = such assemblies so far,
 * out[1] = source entries this rank evaluates (a partition of one rank selects all of them).
 * Round 5, the solve side of the condensed modes and of sparse_multistage (tree engine; reference: the right-hand-side fold and the recovery of the eliminated
 * multipliers, sparse/kkt.hpp:113-175, multistage_kkt.hpp:234-287): the refinement residual is sharded there as well -- x rows and rows of the block that stays in
 * the system by the rank that eliminates them, rows of an eliminated block by every rank that eliminates an x column they touch.  A backend solve on that residual
 * folds it into this rank's x rows only and recovers the eliminated multipliers on those constraint rows only; at the end of a pq_kkt_system_solve that took at
 * least one refinement step the eliminated multipliers cross the ranks once, each row from its owner rank (which = 2 again; sizes_out[2] covers both uses).
 * pq_kkt_sharded_solve_calls: out[0] sharded residual evaluations, [1] rows of the residual in this rank's share (of n + p + m), [2] backend solves that folded /
 * recovered on this rank's rows only, [3] gathers of the multipliers, [4] x rows folded per such solve, [5] constraint rows recovered per such solve. */
int pq_kkt_set_exchange_norm(pq_kkt *k, double *buf_norm);
int pq_kkt_sharded_calls(pq_kkt *k, int out[2]);
int pq_kkt_sharded_solve_calls(pq_kkt *k, int out[6]);
/* test hook (reference-order engine, PQ_SPARSE_LDLT_EXACT): the factor as sparse/ldlt.hpp:24-37 holds it.  what = 0 nnz(L) | 1 L_cols[N + 1] | 2 L_ind | 3 L_vals |
 * 4 D | 5 D_inv | 6 values of P K P' (CSC order of pq_sparse_kkt_symbolic's PKp / PKi_rows) | 7 perm | 8 .. 17 timelines and schedule of the last factorisation / solve
 * (PIQP_AMD_DEBUG=exact_trace, tools/exact_trace.py); copies the item into out_host (NULL: size only) and returns its length, < 0 on error (another engine) */
long long pq_kkt_exact_factor(pq_kkt *k, int what, void *out_host);
/* test hook (sparse backends): smallest |pivot| of the last factorisation */
int pq_kkt_min_abs_pivot(pq_kkt *k, double *out);
/* collectives the native transport has enqueued so far: out[which] for which = 0, 1, 2 (test / bench bookkeeping) */
int pq_kkt_native_exchange_calls(pq_kkt *k, int out[3]);
/* which transport a partitioned handle uses and what its communicator says about itself: out[0] = 0 none / 1 callback / 2 native RCCL; for the native
 * transport out[1..3] = ncclCommCount, ncclCommUserRank, ncclCommCuDevice of the library's communicator (-1 otherwise) -- the figures a multi-GPU
 * bench line carries so that "RCCL saw N ranks" can be checked from the outside */
int pq_kkt_comm_info(pq_kkt *k, int out[4]);
/* what the partition looks like: out[0] = supernodes owned by this rank, out[1] = shared supernodes, out[2] = boundary
 * subtree roots, out[3..4] = this rank's column span, out[5] = work share of this rank in permille, out[6] = shared
 * (replicated) work in permille */
int pq_kkt_partition_info(pq_kkt *k, int out[8]);
/* host-only planning hook for tests (no GPU needed): analyses the KKT pattern of `mode` (0 full .. 3 all eliminated)
 * and writes the owning rank of every permuted column (-1 = shared top) into owner_out[N]; returns N */
int pq_sparse_partition_plan(const pq_sparse_data *data, int mode, int world, int *owner_out, int capacity,
                             double *work_out /* world + 1: per rank, then shared */);

/* ---- the integer work of sparse::KKT's constructor, host-only (no GPU needed), exported so that the index work of the product can be pinned bit for
 * bit (tests/test_symbolic_parity.py: the reference's exact 4 x 4 case, tests/src/sparse/utils_test.cpp:55-92, and the oracle on the frozen fixtures).
 * pq_sparse_amd_order: Eigen-style approximate minimum degree on the pattern of the upper-triangular CSC matrix (sparse/ordering.hpp:67-84: the
 *   `P_eigen.indices()` of AMDOrdering::init, perm[new] = old).
 * pq_sparse_permute_sym_upper: permute_sparse_symmetric_matrix (sparse/utils.hpp:32-128): C = upper(P A P') for perm_inv[old] = new, with the map
 *   Ai_to_Ci of value positions (its return value); Cp[n + 1], Ci[nnz], Ai_to_Ci[nnz].
 * pq_sparse_kkt_symbolic: create_kkt_matrix of `mode` (kkt_full.hpp:39-170 and the three eliminated variants; 0 full, 1 eq, 2 ineq, 3 all) followed by
 *   the two steps above exactly as sparse/kkt.hpp:51-70 runs them.  Call with all outputs NULL to get sizes: returns N and writes nnz(K) to *nnz_out.
 *   Kp[N + 1], Ki[nnz], perm[N] (the AMD ordering), PKp[N + 1], PKi_rows[nnz] (pattern of PKPt), PKi[nnz] (K value index -> PKPt value index).
 * pq_kkt_sparse_ordering (sparse backends, after create): what the handle actually eliminates in.  fill_perm[N] = the fill-reducing ordering chosen
 *   (AMD as above, or nested dissection; perm[new] = old), elim_perm[N] = the same composed with the assembly-tree postorder / leaf amalgamation the
 *   device schedule uses (any postorder of the elimination tree has the same fill), returns 0 = amd, 1 = nested dissection, < 0 on error. */
int pq_sparse_amd_order(int n, const int *Ap, const int *Ai, int *perm);
int pq_sparse_permute_sym_upper(int n, const int *Ap, const int *Ai, const int *perm_inv, int *Cp, int *Ci, int *Ai_to_Ci);
int pq_sparse_kkt_symbolic(const pq_sparse_data *data, int mode, int *nnz_out, int *Kp, int *Ki, int *perm, int *PKp, int *PKi_rows,
                           int *PKi);
int pq_kkt_sparse_ordering(pq_kkt *k, int *fill_perm, int *elim_perm);
/* host-only planning hook of the reference-order engine (PQ_SPARSE_LDLT_EXACT; no GPU needed): everything sparse/ldlt.hpp:42-169 decides from the pattern of the
 * KKT_FULL matrix alone, and the schedule the device kernels replay it with (csrc/sparse_symbolic.hpp, struct UpLooking).  Items (int32 arrays unless noted):
 *   0 stats { nnz(L), tasks, tree height, dependent steps on the longest root path, nnz(K), tickets }   1 perm[N] (AMD, perm[new] = old)
 *   2 Cp[N + 1]  3 Ci[nnz(K)] (pattern of P K P')   4 diag_pos[N]   5 etree[N]   6 Lp[N + 1]   7 Li[nnz(L)] (L in CSC, rows ascending)
 *   8 Rp[N + 1]  9 Rcol  10 Rpos (row k of L in the reference's visiting order: column, CSC position)
 *   11 task_ptr  12 task_rows (tasks = paths of the elimination tree of at most 64 rows)   13 row_task  14 row_lane  15 row_prev
 *   16 dep_ptr  17 dep (children a row pass waits for)   18 tk_kind  19 tk_id (tickets: 0 row pass of a row, 1 path pass of a task)
 *   20 Rcnt  21 Rtab (per entry: leading column entries the row pass scatters, -1 = own path; table row)   22 tab_ptr  23 mask_ptr  24 task_nU
 *   25 Tmask (uint64: presence bits of every table row)
 *   100 + mode (mode = KKTMode bits: 1 equalities eliminated, 2 inequalities eliminated): { N, nnz(L), kiloflops of the factorisation } of that mode's system -- what the
 *       engine choice of pq_kkt_create_sparse looks at (PIQP_AMD_EXACT_MAX_N, PIQP_AMD_EXACT_MAX_FLOPS)
 * len[q] receives the length of item what[q]; out[q] (may be NULL, as may `out`) receives a copy.  Returns N. */
int pq_sparse_uplooking_plan(const pq_sparse_data *data, int nitems, const int *what, void **out, long long *len);

/* measurement hooks: when enabled, the backend brackets its stages with hipEvents on its own stream.
 * stage 0 = KKT assembly kernel (dense: k_syrk_lower<ASSEMBLE>), 1 = factorisation (all panels),
 * 2 = backend solve.  enable = 2 (dense backend, measurement passes only) also brackets individual launches: 3 = fused trailing update +
 * next diagonal block, 4 = panel solve, 5 = both triangular sweeps.  pq_kkt_get_profile returns the accumulated milliseconds / call count
 * and resets them. */
int pq_kkt_set_profiling(pq_kkt *k, int enable);
int pq_kkt_get_profile(pq_kkt *k, int stage, double *total_ms, int *count);

/* ===================== KKTSystem: replaces piqp::KKTSystem<T,I,MatrixType> ===================== */
typedef struct pq_kktsys pq_kktsys;

/* KKTSystem::init, kkt_system.hpp:97-132 (+ backend factory :455-497 keyed by settings->kkt_solver) */
int pq_kktsys_create_dense(pq_kktsys **out, const pq_dense_data *data, const pq_settings *settings, int device);
int pq_kktsys_create_sparse(pq_kktsys **out, const pq_sparse_data *data, const pq_settings *settings, int device);
int pq_kktsys_clone(const pq_kktsys *k, pq_kktsys **out); /* kkt_system.hpp:70-95 */
void pq_kktsys_destroy(pq_kktsys *k);
int pq_kktsys_set_pointer_mode(pq_kktsys *k, int mem);
pq_kkt *pq_kktsys_backend(pq_kktsys *k); /* borrowed */
/* kkt_system.hpp:134-141 */
int pq_kktsys_update_data_dense(pq_kktsys *k, const pq_dense_data *data, int options);
int pq_kktsys_update_data_sparse(pq_kktsys *k, const pq_sparse_data *data, int options);
/* kkt_system.hpp:143-211; returns 1 ok / 0 factor failed */
int pq_kktsys_update_scalings_and_factor(pq_kktsys *k, int iterative_refinement, double rho, double delta,
                                         const pq_vars *vars);
/* kkt_system.hpp:213-369 incl. the iterative-refinement loop (:256-301) run against device-resident
 * vectors; returns 1 ok / 0 (non-finite).  lhs buffers are written in place (never swapped). */
int pq_kktsys_solve(pq_kktsys *k, const pq_vars *rhs, pq_vars *lhs);
/* kkt_system.hpp:392-425 rhs = K_full * lhs */
int pq_kktsys_mul(pq_kktsys *k, const pq_vars *lhs, pq_vars *rhs);
/* diagnostics of the last solve: refinement steps taken, backend solves, final refine error, rhs norm */
int pq_kktsys_last_solve_stats(const pq_kktsys *k, int *refine_steps, int *backend_solves, double *refine_error,
                               double *rhs_norm);
/* ||rhs_bar - K_cond * lhs||_inf and ||rhs_bar||_inf of the last solve, recomputed on device via
 * mul_condensed_kkt (kkt_system.hpp:507-536); the harness's parity metric (SURVEY.md 8b last row) */
int pq_kktsys_condensed_residual(pq_kktsys *k, double *res_inf, double *rhs_inf);
/* test read-back of a state vector into HOST memory, after the handle's stream: x_reg (n; static regularisation of the refinement branch included), z_reg (m; without
 * it), rhs_x_bar (n), rhs_z_bar (m) and lhs_z (m) of the last solve.  PQ_ERR_INVALID before the first factorisation, and for the last three before the first solve. */
enum { PQ_KKTSYS_X_REG = 0, PQ_KKTSYS_Z_REG = 1, PQ_KKTSYS_RHS_X_BAR = 2, PQ_KKTSYS_RHS_Z_BAR = 3, PQ_KKTSYS_LHS_Z = 4 };
int pq_kktsys_state(pq_kktsys *k, int what, double *out_host);
int pq_kktsys_synchronize(pq_kktsys *k);

/* ===================== Solver: piqp::DenseSolver / SparseSolver front-end (caller of the hot path) ===== */
typedef struct pq_solver pq_solver;

int pq_solver_create(pq_solver **out, int device);
void pq_solver_destroy(pq_solver *s);
int pq_solver_clone(const pq_solver *s, pq_solver **out);
pq_settings *pq_solver_settings(pq_solver *s); /* solver.hpp:65 settings() */
/* DenseSolver::setup, solver.hpp:1266-1277: P n x n, A p x n, G m x n column-major HOST arrays;
 * NULL = nullopt.  Returns 1 when setup_done. */
int pq_solver_setup_dense(pq_solver *s, int n, int p, int m, const double *P, const double *c, const double *A,
                          const double *b, const double *G, const double *h_l, const double *h_u, const double *x_l,
                          const double *x_u);
/* ---- problem data that already lives in GPU memory, results returned there ----
 * The *_mem entry points below are the calls above / below them with two more arguments; pq_solver_setup_dense, pq_solver_update_dense, pq_solver_get_result,
 * pq_batch_setup_sparse, pq_batch_update, pq_batch_update_data and pq_batch_get_result forward to them with PQ_MEM_HOST (and PQ_COL_MAJOR).
 *   mem     PQ_MEM_HOST, or PQ_MEM_DEVICE: EVERY non-NULL array pointer of the call is device memory on the handle's device.
 *   layout  storage order of the matrices P (n x n), A (p x n), G (m x n) only: PQ_COL_MAJOR, or PQ_ROW_MAJOR (what a contiguous torch tensor is).  The solver
 *           keeps upper(P), A^T, G^T column-major: a row-major A already is the column-major A^T (plain copy), a column-major one goes through a transpose
 *           kernel; P goes through a masked copy (column-major) or a masked transpose (row-major).
 *   Only the upper triangle of P is read (solver.hpp:169-192), in either layout and either memory: whatever lies in the other triangle -- NaN included --
 *   never reaches the solver.
 *   Any other value of mem or layout returns PQ_ERR_INVALID and leaves the handle as it was.
 * Ordering contract: the caller makes the inputs visible before the call (device mode: the work that produces them has completed, e.g. the producing stream was
 * synchronised).  The call returns only when the library has finished reading them; for results, only when the outputs are written.  Inputs are never modified.
 * Device mode moves no matrix across the host-device link: the matrices go from the caller's arrays into the solver's own by kernel / device-to-device copy,
 * HostData::P_utri / AT / GT are never sized.  The vectors c, b, h_l, h_u, x_l, x_u (O(n + p + m)) are fetched into host staging and go through the same host
 * logic as in host mode (finite-bound index lists, rows of G without a finite bound), so the two modes compute bit for bit the same.  Exception: under
 * PIQP_AMD_DEBUG=host_ruiz (the debugging path that equilibrates on the host) a device-mode call fetches the matrices to the host.
 * pq_solver_last_ingest: figures of the last setup / update of a dense solver (sparse: see pq_solver_setup_sparse), computed from the shapes of the matrices each path moves (not counted by the
 * runtime): out[0] = bytes of matrix data that cross the host-device link (host mode: 8 n (n + p + m) for a setup, 8 n x the columns of the updated matrices for
 * an update; device mode: 0), out[1] = bytes of matrix data written device-to-device or by kernel. */
enum { PQ_COL_MAJOR = 0, PQ_ROW_MAJOR = 1 };
int pq_solver_setup_dense_mem(pq_solver *s, int n, int p, int m, const double *P, const double *c, const double *A,
                              const double *b, const double *G, const double *h_l, const double *h_u, const double *x_l,
                              const double *x_u, int mem, int layout);
int pq_solver_update_dense_mem(pq_solver *s, const double *P, const double *c, const double *A, const double *b,
                               const double *G, const double *h_l, const double *h_u, const double *x_l,
                               const double *x_u, int mem, int layout);
/* the ten solution vectors into host or device buffers (NULL fields skipped).  The dense solver keeps its solution (unscaled, boxes expanded) on the host, so in
 * device mode these O(n + p + m) doubles cross the link host-to-device; only the batched solver's results (pq_batch_get_result_mem) never leave the GPU. */
int pq_solver_get_result_mem(const pq_solver *s, pq_vars *out, int mem);
int pq_solver_last_ingest(const pq_solver *s, long long out[2]);
/* out[] of pq_solver_last_ingest for a sparse solver: out[0] = 8 x the stored nonzeros (upper(P), A, G) of the matrices a host-mode setup / update moves, 0 for a
 * device-mode call; out[1] = bytes written by the gather kernel of a device-mode call.
 * SparseSolver::setup, solver.hpp:1297-1308: CSC HOST arrays (P full or upper) */
int pq_solver_setup_sparse(pq_solver *s, int n, int p, int m, const int *Pp, const int *Pi, const double *Px,
                           const double *c, const int *Ap, const int *Ai, const double *Ax, const double *b,
                           const int *Gp, const int *Gi, const double *Gx, const double *h_l, const double *h_u,
                           const double *x_l, const double *x_u);
/* DenseSolver::update, solver.hpp:1279-1290 */
int pq_solver_update_dense(pq_solver *s, const double *P, const double *c, const double *A, const double *b,
                           const double *G, const double *h_l, const double *h_u, const double *x_l,
                           const double *x_u);
int pq_solver_update_sparse(pq_solver *s, const int *Pp, const int *Pi, const double *Px, const double *c,
                            const int *Ap, const int *Ai, const double *Ax, const double *b, const int *Gp,
                            const int *Gi, const double *Gx, const double *h_l, const double *h_u,
                            const double *x_l, const double *x_u);
/* ---- sparse problem data whose VALUES already live in GPU memory ----
 * pq_solver_setup_sparse / pq_solver_update_sparse with one more argument; they forward here with PQ_MEM_HOST.  mem = PQ_MEM_DEVICE: Px, Ax, Gx and the six vectors
 * are device memory on the handle's device; the index arrays Pp, Pi, Ap, Ai, Gp, Gi are HOST memory in either mode.  Ordering contract, treatment of the vectors
 * (fetched, same host logic, so both modes compute bit for bit the same) and the PIQP_AMD_DEBUG=host_ruiz exception: as written above pq_solver_setup_dense_mem.
 * Any other value of mem returns PQ_ERR_INVALID and leaves the handle as it was.
 * Device mode: at setup, gather maps are built from the patterns alone -- stored entry of upper(P) <- the caller's entry on or above the diagonal (rows ascending
 * within a column), stored entry of A^T / G^T <- the caller's CSC entry of A / G -- and from then on only values move: a gather kernel (csrc/ingest_kernels.hip)
 * fills the solver's device arrays, the rows of G without a finite bound are zeroed by a kernel, unscale_data -> assign -> scale_data (sparse/preconditioner.hpp)
 * run on those arrays, and the KKT backend is refreshed from a device-mode pq_sparse_data.  No matrix value comes to the host or crosses the link; entries of P
 * below the diagonal are never loaded (NaN there is harmless).  In pq_solver_update_sparse_mem with PQ_MEM_DEVICE the index arrays may be NULL: identical sparsity is
 * the reference's precondition (solver.hpp:325,341,356), the value arrays are read in the CSC order given at setup.  Lengths: the caller guarantees that Px, Ax,
 * Gx hold as many entries as the arrays given at setup (Pp[n], Ap[n], Gp[n] of that call); where index arrays are passed their totals are checked against those
 * counts (the host path's per-column check of P has no counterpart: the map fixes which entries are read), where they are NULL nothing can be checked.
 * Where the values live is a one-way switch: a host-fed solver keeps a host mirror of its values until its first device-mode update, which drops the mirror for the
 * rest of the handle's life; from then on, as for a solver set up in device mode, a host-mode update stages the caller's values in device memory and takes the
 * device path (out[0] of pq_solver_last_ingest counts them; the same length guarantee holds for the host arrays).  Results do not depend on the switch.
 * pq_debug_sparse_ingest_maps (host-only, no GPU needed): those maps in scatter form for tests -- mapP[k] / mapA[k] / mapG[k] = stored position of the caller's
 * entry k in upper(P) / A^T / G^T, -1 = never read; NULL Ap / Gp = absent matrix, NULL map = skipped; nnz_out = stored entries of the three.  Returns 0. */
int pq_solver_setup_sparse_mem(pq_solver *s, int n, int p, int m, const int *Pp, const int *Pi, const double *Px,
                               const double *c, const int *Ap, const int *Ai, const double *Ax, const double *b,
                               const int *Gp, const int *Gi, const double *Gx, const double *h_l, const double *h_u,
                               const double *x_l, const double *x_u, int mem);
int pq_solver_update_sparse_mem(pq_solver *s, const int *Pp, const int *Pi, const double *Px, const double *c,
                                const int *Ap, const int *Ai, const double *Ax, const double *b, const int *Gp,
                                const int *Gi, const double *Gx, const double *h_l, const double *h_u,
                                const double *x_l, const double *x_u, int mem);
int pq_debug_sparse_ingest_maps(int n, int p, int m, const int *Pp, const int *Pi, const int *Ap, const int *Ai,
                                const int *Gp, const int *Gi, int *mapP, int *mapA, int *mapG, int nnz_out[3]);
int pq_solver_solve(pq_solver *s);               /* solver.hpp:69-148; returns Status */
const pq_info *pq_solver_info(const pq_solver *s); /* result().info */
/* result(): copies the ten solution vectors (sizes n,p,m,m,n,n,m,m,n,n) into host buffers (NULL skipped) */
int pq_solver_get_result(const pq_solver *s, pq_vars *out_host);
int pq_solver_dims(const pq_solver *s, int *n, int *p, int *m);
/* optional per-iteration trace (rows of 11 doubles = the verbose table, solver.hpp:590-602) */
int pq_solver_set_trace(pq_solver *s, double *buf_host, int max_rows);
int pq_solver_trace_rows(const pq_solver *s);
/* pq_kkt_partition / pq_kkt_set_exchange on the solver's KKT backend (after setup): the interior-point loop then runs
 * replicated on every rank, bit for bit the same, with the factor / solve work split across the ranks */
int pq_solver_partition(pq_solver *s, int rank, int world, long long sizes_out[3]);
int pq_solver_set_exchange(pq_solver *s, pq_exchange_fn exchange, void *user, double *buf_factor, double *buf_forward,
                           double *buf_gather);
int pq_solver_set_comm_rccl(pq_solver *s, const unsigned char id[128], int rank, int world);
int pq_solver_native_exchange_calls(pq_solver *s, int out[3]);
int pq_solver_set_exchange_norm(pq_solver *s, double *buf_norm); /* as pq_kkt_set_exchange_norm */
int pq_solver_sharded_calls(pq_solver *s, int out[2]);
int pq_solver_sharded_solve_calls(pq_solver *s, int out[6]);
int pq_solver_comm_info(pq_solver *s, int out[4]); /* as pq_kkt_comm_info */

/* ===================== Batched solver: many structurally identical sparse QPs in one launch ===================== */
/* The reference has no batch API (one SolverBase per QP, solver.hpp:42); this is the device-side equivalent of
 *     for (i < batch) { SparseSolver s; s.settings() = settings; s.setup(P_i, c_i, A_i, ...); s.solve(); }
 * with kkt_solver = sparse_multistage (the default of pq_batch_create), sparse_ldlt or sparse_ldlt_exact: one workgroup runs the whole
 * interior-point method (solver.hpp:379-1259) of one QP, the batch is the grid.  All instances share the sparsity patterns and, unless
 * pq_batch_set_bound_sets says otherwise, the set of finite bounds.  settings->kkt_solver, read by pq_batch_setup_sparse, picks the KKT backend of the handle:
 *   PQ_SPARSE_MULTISTAGE                    the multistage chain Cholesky (sparse/multistage_kkt.hpp) of the stage structure found in the pattern;
 *   PQ_SPARSE_LDLT / PQ_SPARSE_LDLT_EXACT   the reference's sparse_ldlt: the full KKT matrix in AMD order, up-looking LDLt (sparse/kkt.hpp, ldlt.hpp),
 *                                           every factor and every solve bitwise the reference's; one 64-thread workgroup per QP, n + p + m <= 8192.
 * Every other value (condensed modes, dense, multifrontal) is refused at setup. */
typedef struct pq_batch pq_batch;

int pq_batch_create(pq_batch **out, int device);
void pq_batch_destroy(pq_batch *s);
pq_settings *pq_batch_settings(pq_batch *s); /* solver.hpp:65 settings(), shared by all instances */
/* A second handle in the state of s, without a new setup, under the rules of pq_solver_batch_clone / _clone_select: the whole batch (_clone: the identity list) or
 * a list of instances (_clone_select: batch = count, instance j of the new handle is instance idx[j] of s; idx in HOST memory, repeats allowed, count smaller or
 * larger than the batch of s).  Copied: the settings as they stand, the bound-set mode, the start-order flag.  Per instance everything a later call can read goes
 * along bit for bit -- the arena row (scaled data, the stored Ruiz scalings, x_b_scaling, the interior-point state, the ten result vectors, the grouped-row and
 * front arenas of sparse_multistage, C / L / D / D^-1 of sparse_ldlt), its cost scaling, its pq_info, its profile row and, with PQ_BOUND_SETS_PER_INSTANCE, its
 * lists with the dropped flags.  So a clone taken after a solve answers pq_batch_info, pq_batch_get_result(_mem) and pq_batch_get_profile without solving, after a
 * pq_batch_kkt_factor it answers pq_batch_ldlt_factor and pq_batch_kkt_solve, and an update on it unscales with the stored scalings of its instances.  The patterns,
 * the symbolic analysis, the update maps and the shared bound lists are those of s: nothing is analysed again, no host data are needed, and their device arrays,
 * which no kernel writes, are held by both handles and released by the last one.  The new handle is on the same device with a stream of its own and is
 * independent: it survives pq_batch_destroy(s) and a new pq_batch_setup_sparse on s, and no call on either is seen by the other; s is only waited for and read.
 * The MODE_WAVE kernel variant (waves per SIMD) is chosen for count, as setup chooses it for its batch; the start order of the next launch is computed from the
 * gathered infos as pq_batch_solve leaves it.  The call is the only one on the new handle that allocates beyond what the same call allocates after a setup; the
 * sparse_ldlt backend repeats setup's free-memory refusal for the new arena.  One gather launch for the arena (16-byte words; 8 with an odd row), one for each of
 * the small per-instance arrays; the call ends with a wait.
 * _clone of a handle that was never set up gives a handle with the copied scalars and no problem; _clone_select of one is PQ_ERR_INVALID, as are, before any device
 * call and with *out left alone: a NULL s, out or idx, count < 1, an idx[j] outside [0, batch) (the text names j and the value). */
int pq_batch_clone(const pq_batch *s, pq_batch **out);
int pq_batch_clone_select(const pq_batch *s, const int *idx, int count, pq_batch **out);
/* of the clone call that made s: out2 = { wall ms of the call, device ms of the gathers (hipEvents of the new handle around them) }; both 0 on a handle that
 * pq_batch_create made or whose source was never set up.  Wall minus device is the allocation, the host images and the waits. */
int pq_batch_clone_ms(const pq_batch *s, double out2[2]);
/* measurement and test hook: the doubles of one instance's row of the arena -- what a clone gathers per instance, 8 x this many bytes read and as many written; 0
 * before a setup, PQ_ERR_INVALID for a NULL handle.  Even at every shape (every slot of the row is padded to an even count), so rows are 16-byte aligned. */
long long pq_batch_arena_stride(const pq_batch *s);
/* Who owns the set of finite bounds: PQ_BOUND_SETS_SHARED (the default) or PQ_BOUND_SETS_PER_INSTANCE, the constants and their meaning as at
 * pq_solver_batch_set_bound_sets.  Shared: setup refuses an instance whose finite bounds differ from instance 0's and the updates refuse a bound that turns
 * finite or infinite.  Per instance: every instance has the lists SparseSolver would hold for its own vectors (sparse/data.hpp:103-210) at setup and after every
 * update, so a row of G or a box can be switched off in some instances with -/+ infinity and come back later; nothing is refused on finiteness.  The mode is read by
 * pq_batch_setup_sparse; a handle that is set up keeps the mode its setup read.  The kernel variant, the working-set mode and the threads per QP do not depend on
 * it.  PQ_ERR_INVALID for a NULL handle or any other value.
 * UPDATES IN PER-INSTANCE MODE (pq_batch_update, pq_batch_update_data and their _mem forms): the lists the reference would hold after the call REPLACE the
 * instance's own, by the rules stated at pq_solver_batch_update_dense -- set_h_l / set_h_u with the given vector for a given side and the stored finiteness for the
 * other, a row dropped earlier being stored finite on both sides as -1 / 1; then disable_inf_constraints, set_x_l, set_x_u; a given box vector is packed to its
 * new list; a stored infinite bound IS infinite.  The lists are built by a kernel on the vectors where they are: in device mode nothing is allocated and no
 * vector crosses the link.  Two behaviours follow from this solver keeping ONE copy of G', from which every KKT matrix is assembled:
 *   1. A row dropped by an update WITHOUT G values has its entries of G' zeroed in that copy (and, multistage backend, in the grouped-row arena the fronts are
 *      assembled from), so the KKT backend sees the row gone.  The reference zeroes GT but does not tell its KKT backend, which keeps factorising the old row
 *      against the bounds -1 / 1.  The state here is the reference's after update(G = its own G, h_l, h_u, ...) with preconditioner_reuse_on_update = 1, up to the
 *      roundings of its unscale / rescale.
 *   2. A row that comes back keeps zero entries of G' until G values are given, as in the reference: pass Gx together with bounds that re-enable a row, or the row
 *      reads h_l <= 0 <= h_u.  Values of G given for a row that is dropped (now, or by the same call) are not stored. */
int pq_batch_set_bound_sets(pq_batch *s, int mode);
/* test hook: the lists the handle holds for one instance NOW (in shared mode: the shared ones), read back from the device tables the kernels use, to HOST memory.
 * counts = n_h_l, n_h_u, n_x_l, n_x_u; the four ascending lists ([m], [m], [n], [n]; counts[k] entries are written); dropped [m]: 1 on the rows of G without a
 * finite bound, whose entries of G' are zeroed (such a row is in both lists, with the bounds -1 / 1).  Any output but counts may be NULL. */
int pq_batch_bound_lists(const pq_batch *s, int instance, int counts[4], int *h_l_idx, int *h_u_idx, int *x_l_idx, int *x_u_idx, int *dropped);
/* SparseSolver::setup (solver.hpp:1297-1308) per instance.  Patterns (CSC, HOST): P n x n (upper triangle taken),
 * A p x n, G m x n; NULL pattern = absent.  Values / vectors are [batch][nnz] resp. [batch][len] row-major HOST
 * arrays; NULL h_l/h_u/x_l/x_u = nullopt.  Returns 1 when set up.  Forwards to pq_batch_setup_sparse_mem with PQ_MEM_HOST: the arrays are uploaded into one
 * device staging buffer and the setup reads them there. */
int pq_batch_setup_sparse(pq_batch *s, int batch, int n, int p, int m, const int *Pp, const int *Pi, const double *Px,
                          const double *c, const int *Ap, const int *Ai, const double *Ax, const double *b,
                          const int *Gp, const int *Gi, const double *Gx, const double *h_l, const double *h_u,
                          const double *x_l, const double *x_u);
/* The same with the problem data in host or device memory (mem; ordering contract: see pq_solver_setup_dense_mem; any other value: PQ_ERR_INVALID, the handle
 * as it was).  Both modes are one setup; they differ in how the data reaches the kernels.  The shared structure is analysed from the patterns -- no analysis reads
 * a value -- and from instance 0's h_l, h_u, x_l, x_u; no HostData is built for the instances 1 and up.  With shared bound sets every instance must have instance
 * 0's finiteness pattern ("batch setup: instances differ in which bounds are finite" otherwise); with PQ_BOUND_SETS_PER_INSTANCE a kernel builds the table of
 * every instance's lists (a vector that is not given has no finite entry; a row of G with no finite bound is dropped: in both lists, -1 / 1, its entries of G'
 * zero).  Then kernels fill the zeroed arena from [batch][nnz] / [batch][len] device arrays -- upper(P), A', G' through the entry maps the updates use, the vectors
 * by the rules of set_h_l / set_h_u, the box vectors packed to the lists, x_b_scaling = 1; entries of P below the diagonal are never loaded -- and the
 * equilibration and prepare kernels follow.  The two modes agree bit for bit; so do the refusals and the state of the handle after one: a setup gives up the
 * handle's previous problem when it starts, so a handle whose setup was refused has none.
 * PQ_MEM_DEVICE: Px, Ax, Gx and the six vectors are DEVICE arrays on the handle's device, read where they are; the six index arrays stay HOST memory, as in
 * pq_solver_setup_sparse_mem.  Instance 0's four bound vectors are fetched to the host: 8 x (the lengths of those of the four that are given) bytes, 8 (2 m + 2 n)
 * at most, in either bound-set mode.  Nothing else of the problem data comes to the host and none of it crosses host to device; the finiteness check is a kernel
 * on the caller's arrays (one flag word comes back).
 * PQ_MEM_HOST: nothing is fetched, instance 0's vectors are the first rows of the caller's arrays, and the finiteness check is a host loop that runs before the call
 * allocates anything on the device.  The arrays that are given and not empty are then copied into ONE device staging buffer, which the kernels read; it is
 * released before the call returns, and the call returns only after the copies have read the caller's memory.  Peak device memory of a host-fed setup is so higher
 * by the size of the caller's data (57 MB beside a 692 MB arena for 8192 MPC QPs); the buffer is allocated before the free-memory check of the sparse_ldlt backend,
 * which accounts for it. */
int pq_batch_setup_sparse_mem(pq_batch *s, int batch, int n, int p, int m, const int *Pp, const int *Pi, const double *Px,
                              const double *c, const int *Ap, const int *Ai, const double *Ax, const double *b,
                              const int *Gp, const int *Gi, const double *Gx, const double *h_l, const double *h_u,
                              const double *x_l, const double *x_u, int mem);
/* Figures of the last setup / update of the handle, computed from the shapes of what the call was given (not counted by the runtime).  out[0] = bytes of problem
 * data moved across the host-device link: host mode 8 x batch x the lengths given (nnz of the matrices as the caller passes them), for a setup -- the upload of
 * its staging buffer; nothing is fetched -- as for an update; device mode 0 for an update and the fetch stated at pq_batch_setup_sparse_mem -- device to host -- for
 * a setup.  out[1] = bytes the ingest kernels write into the arena, the same figure in both modes: 8 x batch x (the stored nonzeros of the matrices given + the
 * lengths of the vectors given; a setup writes both bounds of G and x_b_scaling whatever is given: 2 m + n in place of the lengths of h_l, h_u); box vectors count
 * in full although they are packed to their lists.  A NULL handle or out: PQ_ERR_INVALID, out untouched. */
int pq_batch_last_ingest(const pq_batch *s, long long out[2]);
/* Of the last pq_batch_setup_sparse(_mem) of the handle, milliseconds: out3[0] wall time of the call, out3[1] of it the host analysis (symbolic analysis, entry maps,
 * descriptor and tables), out3[2] device time by the handle's events from the fill of the arena (host mode: the staged copies, that is from before the upload of the
 * staging buffer, the host analysis running meanwhile) to the end of the equilibration and prepare kernels.  Zeros before the first setup and on a clone.  A NULL handle or out3: PQ_ERR_INVALID, out3 untouched. */
int pq_batch_setup_ms(const pq_batch *s, double out3[3]);
/* update() of every instance with new VECTORS only (solver.hpp:218-308 with every optional matrix empty; the Ruiz scaling of the
 * setup is reused, :283-285).  [batch][len] HOST arrays, NULL = unchanged.  The set of finite bounds is part of the shared
 * structure and must not change (error otherwise); a doubly-infinite row of G stays as it was at setup.  With PQ_BOUND_SETS_PER_INSTANCE: see
 * pq_batch_set_bound_sets. */
int pq_batch_update(pq_batch *s, const double *c, const double *b, const double *h_l, const double *h_u,
                    const double *x_l, const double *x_u);
/* update() of every instance with new MATRIX VALUES and / or vectors (solver.hpp:218-308 with update_P / update_A / update_G of
 * :317-358).  Px / Ax / Gx: [batch][nnz] HOST arrays in the CSC order of the patterns given at setup (identical sparsity is the
 * reference's precondition too), NULL = unchanged.  Per instance, on the device: unscale_data, assign, scale_data with a fresh Ruiz
 * equilibration (sparse/preconditioner.hpp:65-222) unless settings.preconditioner_reuse_on_update, then the front arenas are rebuilt.
 * With all three matrices NULL this is pq_batch_update.  Returns 1. */
int pq_batch_update_data(pq_batch *s, const double *Px, const double *Ax, const double *Gx, const double *c, const double *b,
                         const double *h_l, const double *h_u, const double *x_l, const double *x_u);
/* pq_batch_update / pq_batch_update_data with the arrays in host or device memory (mem, ordering contract: see pq_solver_setup_dense_mem).  Device mode: the
 * kernels read the caller's [batch][len] / [batch][nnz] arrays in place -- no device allocation (pq_debug_alloc_count does not move), no copy across the link; the
 * check that the set of finite bounds is unchanged runs as a kernel over the caller's arrays and one flag word comes back (same error as in host mode; with
 * PQ_BOUND_SETS_PER_INSTANCE there is no such check, a kernel builds every instance's new lists from the arrays instead). */
int pq_batch_update_mem(pq_batch *s, const double *c, const double *b, const double *h_l, const double *h_u,
                        const double *x_l, const double *x_u, int mem);
int pq_batch_update_data_mem(pq_batch *s, const double *Px, const double *Ax, const double *Gx, const double *c, const double *b,
                             const double *h_l, const double *h_u, const double *x_l, const double *x_u, int mem);
/* solve() of every instance (solver.hpp:69-148); returns the number of instances that ended PQ_SOLVED (>= 0) */
int pq_batch_solve(pq_batch *s);
const pq_info *pq_batch_info(const pq_batch *s, int instance); /* result().info of one instance */
/* result(): field k of Variables (0..9 = x, y, z_l, z_u, z_bl, z_bu, s_l, s_u, s_bl, s_bu) of ALL instances,
 * copied to a HOST array [batch][len] (len = n, p or m) */
int pq_batch_get_result(pq_batch *s, int field, double *out_host);
/* the same into a host or a DEVICE array [batch][len] (device mode: one strided device-to-device copy out of the arena, no allocation) */
int pq_batch_get_result_mem(pq_batch *s, int field, double *out, int mem);
/* ACTING ON A LIST OF INSTANCES, IN PLACE (the _select forms of pq_batch_solve, pq_batch_update_mem, pq_batch_update_data_mem and pq_batch_get_result_mem): the
 * same handle, the same arena, the same result arrays -- no second handle as with pq_batch_clone_select.  idx: `count` instances in HOST memory; the value arrays
 * and out are [count][len] / [count][nnz], row j belongs to instance idx[j]; mem says where the value arrays / out live, as in the _mem calls.
 * A LISTED instance ends in the state the whole-batch call would leave it in when given the same row, bit for bit (arena row, cost scaling, pq_info, profile row,
 * its lists with PQ_BOUND_SETS_PER_INSTANCE): the same kernels run on the same row, one workgroup per listed instance, which finds its instance through the list.
 * Of an UNLISTED instance no byte is written: arena row, cost scaling, device and host pq_info, profile row, row of the bound table.
 * _solve_select: returns how many of the listed instances ended PQ_SOLVED.  The settings as they stand at the call (a straggler is run again in place with another
 * max_iter); invalid settings: the listed infos alone become PQ_INVALID_SETTINGS, 0 is returned.  pq_batch_last_kernel_ms reports this launch.  The kernel variant
 * stays the one the handle chose at setup.  Start order: with pq_batch_set_start_order on, the listed instances that took most iterations in their previous solve
 * first, ties in list order; off: list order; results do not depend on it.  The stored order of the next WHOLE solve stays a permutation of the batch: the list goes
 * into a buffer of its own, and after the call the whole order is recomputed from all infos as pq_batch_solve leaves it.
 * _update_select_mem / _update_data_select_mem: the sequences of pq_batch_update / pq_batch_update_data (unscale, bound lists, assign, equilibrate, prepare) on the
 * listed rows.  Shared bound sets: the finiteness check runs over the `count` rows given, a mismatch is refused with pq_batch_update's text and the handle stays as
 * it was; per-instance sets: the lists of the listed instances are rebuilt and no others.  With Px, Ax and Gx all NULL the data form is the vector form.  An updated
 * instance keeps the results and the info of its last solve until it is solved again, as after the whole-batch calls.  Return 1.
 * _get_result_select_mem: field k (as pq_batch_get_result) of the listed instances -> out [count][len] by one gather kernel; repeats are allowed, count may exceed
 * the batch; a field of length 0 writes nothing and returns 0.
 * ALLOCATION: the first _select call on a handle allocates one int buffer of `batch` entries (setup and clone allocate nothing for it); after that _solve_select
 * and the device-memory forms of the other three allocate nothing (pq_debug_alloc_count does not move); host-memory updates stage [count][len], a host-memory
 * result [count][len].
 * REFUSED with PQ_ERR_INVALID before any device call, the handle untouched, the text naming j and the value where there is one: a NULL s or idx (or out), count < 1,
 * an unknown mem or field, a handle that is not set up, an idx[j] outside [0, batch), and -- _solve_select and the two updates only -- an instance listed twice
 * (two workgroups on one arena row would race). */
int pq_batch_solve_select(pq_batch *s, const int *idx, int count);
int pq_batch_update_select_mem(pq_batch *s, const int *idx, int count, const double *c, const double *b, const double *h_l, const double *h_u,
                               const double *x_l, const double *x_u, int mem);
int pq_batch_update_data_select_mem(pq_batch *s, const int *idx, int count, const double *Px, const double *Ax, const double *Gx, const double *c,
                                    const double *b, const double *h_l, const double *h_u, const double *x_l, const double *x_u, int mem);
int pq_batch_get_result_select_mem(pq_batch *s, const int *idx, int count, int field, double *out, int mem);
/* test hook: one instance's row of the arena, pq_batch_arena_stride() doubles, to HOST memory; PQ_ERR_INVALID for a NULL argument, a handle that is not set up or
 * an instance outside [0, batch) */
int pq_batch_arena_row(const pq_batch *s, int instance, double *out_host);
int pq_batch_dims(const pq_batch *s, int *batch, int *n, int *p, int *m);
int pq_batch_block_info(const pq_batch *s, int *out_host, int capacity); /* as pq_kkt_multistage_block_info; sparse_multistage only (error otherwise) */
/* in-kernel device-clock seconds of one instance's last solve: out8 = {KKT assembly, factorisation (chain / LDLt),
 * substitution (chain / LDLt), KKTSystem::solve total, residual updates, whole solve, 0, 0} */
int pq_batch_get_profile(pq_batch *s, int instance, double *out8);
/* hipEvent time of the last solve's kernel and the workgroup size used per QP */
int pq_batch_last_kernel_ms(const pq_batch *s, double *ms, int *threads_per_qp);
/* start order of the instances inside the launch: 1 (default) = the instances that needed most iterations in the PREVIOUS solve of this handle start first
 * (receding-horizon batches repeat their counts; a batch larger than the device holds at once then ends earlier), 0 = always in index order.  Results do not
 * depend on it. */
int pq_batch_set_start_order(pq_batch *s, int longest_first);
/* sparse_ldlt backend only (error code on a sparse_multistage handle), after setup: the KKT backend on its own, on every instance's stored (scaled) data.
 * pq_batch_kkt_factor = KKTSolverBase::update_scalings_and_factor per instance (delta [batch], x_reg [batch][n], z_reg [batch][m]; ok [batch] out: 0 where a
 * pivot is exactly zero, ldlt.hpp:163); pq_batch_kkt_solve = KKTSolverBase::solve with the last factorisation ([batch][len] HOST arrays).  They run the device
 * functions of pq_batch_solve's kernel, launched on their own. */
int pq_batch_kkt_factor(pq_batch *s, const double *delta, const double *x_reg, const double *z_reg, int *ok);
int pq_batch_kkt_solve(pq_batch *s, const double *rhs_x, const double *rhs_y, const double *rhs_z, double *lhs_x, double *lhs_y,
                       double *lhs_z);
/* the last factor of one instance, what = 0 .. 7 as pq_kkt_exact_factor (0 nnz(L) | 1 L_cols | 2 L_ind | 3 L_vals | 4 D | 5 D_inv | 6 values of P K P' |
 * 7 perm); copies the item into out_host (NULL: size only) and returns its length, < 0 on error */
long long pq_batch_ldlt_factor(const pq_batch *s, int instance, int what, void *out_host);

/* ===================== the dense factorisation classes as objects of their own ===================== */
/* piqp::dense::LDLTNoPivot<Mat, UpLo> (dense/ldlt_no_pivot.hpp:87-262; kind = PQ_DENSE_LDLT_NO_PIVOT) and the Eigen::LLT<Mat, UpLo> that dense/kkt.hpp:82 uses
 * (kind = PQ_DENSE_CHOLESKY), for either triangle: what tests/src/dense/ldlt_test.cpp and benchmarks/src/dense_cholesky_factorization_benchmark.cpp:16-109 exercise.
 * The kernels are the dense KKT backend's; the Upper variants work on the transposed view as ldlt_no_pivot.hpp:357-371 does, so U = L^T bit for bit. */
enum { PQ_LOWER = 1, PQ_UPPER = 2 }; /* Eigen::Lower, Eigen::Upper */
typedef struct pq_dense_factor pq_dense_factor;
int pq_dense_factor_create(pq_dense_factor **out, int device, int n, int kind, int uplo); /* ldlt_no_pivot.hpp:126-131 (preallocating constructor) */
void pq_dense_factor_destroy(pq_dense_factor *f);
/* compute(), ldlt_no_pivot.hpp:393-423: reads the `uplo` triangle of A (column-major, leading dimension lda >= n, in host or device memory per `mem`).
 * Returns info(): 0 = Eigen::Success, 1 = Eigen::NumericalIssue (LDLTNoPivot: an exact zero pivot, :307; LLT: a pivot <= 0), negative = PQ_ERR_*. */
int pq_dense_factor_compute(pq_dense_factor *f, const double *A, int lda, int mem);
int pq_dense_factor_info(const pq_dense_factor *f); /* ldlt_no_pivot.hpp:231 */
/* solveInPlace(), ldlt_no_pivot.hpp:432-450 / 464-470: x[n] <- A^-1 x */
int pq_dense_factor_solve_in_place(pq_dense_factor *f, double *x, int mem);
/* matrixLDLT(), ldlt_no_pivot.hpp:217 (LLT: matrixLLT()): writes the `uplo` triangle of out_host (column-major, leading dimension ldo): the strictly triangular
 * part of unit L (PQ_UPPER: of U = L^T) with D on the diagonal; LLT: L resp. U.  The other triangle of out_host is not touched. */
int pq_dense_factor_matrix(pq_dense_factor *f, double *out_host, int ldo);
/* out2[0]: device time of the factorisation launches of the last compute() (hipEvents), out2[1]: wall time of the whole call (copy + symmetric completion +
 * factorisation + status read-back), both in ms */
int pq_dense_factor_last_ms(const pq_dense_factor *f, double out2[2]);

/* ----- the same two classes for a BATCH of small matrices (n <= PQ_DENSE_FACTOR_BATCH_MAX_N), one launch per compute() and per solve ----- */
/* Every matrix of the batch is factored by one workgroup (n >= 32) or one wave (n < 32) with the matrix resident in LDS, in the reference's own order of
 * floating-point operations (csrc/dense_factor_batch.hip): per matrix the factor, the status and every solve are those of the CPU oracle's restatement of the
 * two classes (oracle/orc_dense.c), bit for bit.  The instances share nothing: a failing matrix ends alone. */
enum { PQ_DENSE_FACTOR_BATCH_MAX_N = 128 };
typedef struct pq_dense_factor_batch pq_dense_factor_batch;
/* ldlt_no_pivot.hpp:126-131 (preallocating constructor), `batch` times: everything the handle will ever need, the staging of host-mode calls (up to max_nrhs
 * right-hand sides per matrix) included -- pq_debug_alloc_count() does not move after it.  Arguments are checked before the device is touched: PQ_ERR_UNSUPPORTED
 * for n > PQ_DENSE_FACTOR_BATCH_MAX_N, PQ_ERR_INVALID for batch < 1, n < 1, max_nrhs < 1, a kind that is neither PQ_DENSE_CHOLESKY nor PQ_DENSE_LDLT_NO_PIVOT, an
 * uplo that is neither PQ_LOWER nor PQ_UPPER, a null out. */
int pq_dense_factor_batch_create(pq_dense_factor_batch **out, int device, int batch, int n, int kind, int uplo, int max_nrhs);
void pq_dense_factor_batch_destroy(pq_dense_factor_batch *f);
/* compute(), ldlt_no_pivot.hpp:393-423 / Eigen::LLT::compute, per matrix: matrix i is column-major at A + i * stride (leading dimension lda >= n,
 * stride >= lda * n doubles; host or device memory per `mem`); only its `uplo` triangle is read.  Returns the number of matrices that ended with Eigen::Success
 * (negative = PQ_ERR_*), when the factors are complete. */
int pq_dense_factor_batch_compute(pq_dense_factor_batch *f, const double *A, int lda, long long stride, int mem);
/* info(), ldlt_no_pivot.hpp:231, per matrix: info_host[batch] = 0 (Eigen::Success) / 1 (Eigen::NumericalIssue); first_bad_col_host[batch] (may be NULL) = -1 or
 * the column at which the routine gives up (ldlt_no_pivot.hpp:307 an exact zero pivot; Eigen LLT.h unblocked: a pivot that is not positive) */
int pq_dense_factor_batch_info(const pq_dense_factor_batch *f, int *info_host, int *first_bad_col_host);
/* solveInPlace(MatrixBase&), ldlt_no_pivot.hpp:464-470 (the sweeps of :432-450 per column) / Eigen::LLT::solveInPlace: matrix i's right-hand sides are n x nrhs
 * column-major at X + i * stride, leading dimension ldx >= n, stride >= ldx * nrhs; nrhs <= max_nrhs.  The block of a matrix whose factorisation failed is left as
 * it was.  PQ_ERR_INVALID before the first compute(). */
int pq_dense_factor_batch_solve_in_place(pq_dense_factor_batch *f, double *X, int ldx, int nrhs, long long stride, int mem);
/* matrixLDLT() (ldlt_no_pivot.hpp:217) / matrixLLT() of one instance, as pq_dense_factor_matrix: the `uplo` triangle of out_host (column-major, ldo >= n) */
int pq_dense_factor_batch_matrix(pq_dense_factor_batch *f, int instance, double *out_host, int ldo);
/* out2[0]: device time of the factorisation launch of the last compute() (hipEvents), out2[1]: wall time of the whole call, both in ms */
int pq_dense_factor_batch_last_ms(const pq_dense_factor_batch *f, double out2[2]);

/* ===================== the dense KKT backend for a BATCH of small QPs (n <= PQ_KKT_BATCH_DENSE_MAX_N) ===================== */
/* `batch` independent instances of piqp::dense::KKT (dense/kkt.hpp:39-160) that share n, p, m and the factorisation kind: kkt_solver = PQ_DENSE_CHOLESKY
 * (Eigen::LLT) or PQ_DENSE_LDLT_NO_PIVOT, both in the reference's own order of floating-point operations (csrc/dense_kkt_batch.hip).  Per instance the assembled
 * matrix P + diag(x_reg) + AT AT'/delta + GT diag(1/z_reg) GT', its factor, the success flag, every solve and the three mat-vec evaluators are those of the CPU
 * oracle's dense backend (oracle/orc_dense.c) bit for bit.  The instances share nothing: a failing instance ends alone.  n <= 128 because the n x n square of an
 * instance lives in LDS; p >= 0 and m >= 0 are not limited (AT and GT stay in global memory).
 * Data layout: pq_dense_data's, `batch` times, contiguous: P_utri[i] column-major n x n at P_utri + i n n (only its upper triangle is read: NaN in the other one is
 * harmless), AT[i] column-major n x p at AT + i n p, GT[i] column-major n x m at GT + i n m.  Vectors are [batch][len], per-instance scalars (delta, alpha*) [batch].
 * mem (pq_mem) says where EVERY array argument of that call lives; ordering contract: see pq_solver_setup_dense_mem.  The handle keeps its own device copy of the
 * data (device mode: copied device-to-device, nothing crosses the link). */
enum { PQ_KKT_BATCH_DENSE_MAX_N = 128 };
typedef struct pq_kkt_batch pq_kkt_batch;
/* Arguments are checked before the device is touched: PQ_ERR_UNSUPPORTED for n > PQ_KKT_BATCH_DENSE_MAX_N; PQ_ERR_INVALID for batch < 1, n < 1, p < 0, m < 0, a
 * kkt_solver other than the two, a mem other than the two, a null out or P_utri, a null AT with p > 0 or a null GT with m > 0.  Allocates everything the handle will
 * ever need (the staging of host-mode calls included: pq_debug_alloc_count() moves in no later call except pq_kkt_batch_clone / _clone_select) and computes AT_A[i] = AT[i] AT[i]'
 * (dense/kkt.hpp:53) when p > 0. */
int pq_kkt_batch_create_dense(pq_kkt_batch **out, int device, int batch, int n, int p, int m, int kkt_solver, const double *P_utri, const double *AT,
                              const double *GT, int mem);
void pq_kkt_batch_destroy(pq_kkt_batch *k);
int pq_kkt_batch_clone(const pq_kkt_batch *k, pq_kkt_batch **out);
/* Clone by a list of instances: the new handle has batch = count and its instance j is instance idx[j] of k -- its data, A'A, its stored factor, the scalings of
 * its last factorisation and its status, bit for bit, so a clone taken after a factorisation solves without factoring.  idx: HOST memory in either mode, repeats
 * allowed, count smaller or larger than k's batch.  The new handle lives on the same device with a stream of its own and is independent of k, which is only waited
 * for and read.  One gather launch per buffer (the status is two arrays in one buffer: two), the list uploaded once; the staging and the events are sized for
 * count, not copied.  The call allocates everything the new handle will ever need.  PQ_ERR_INVALID before the device is touched, with *out left alone: a NULL k,
 * out or idx, count < 1, an idx[j] outside [0, batch) (the text names j and the value). */
int pq_kkt_batch_clone_select(const pq_kkt_batch *k, const int *idx, int count, pq_kkt_batch **out);
int pq_kkt_batch_dims(const pq_kkt_batch *k, int *batch, int *n, int *p, int *m);
/* dense/kkt.hpp:62-71, per instance.  options: PQ_KKT_UPDATE_* mask; a flagged matrix is re-read from its argument (null there: PQ_ERR_INVALID, the handle stays as
 * it was), an unflagged one is ignored and its pointer may be null; PQ_KKT_UPDATE_A recomputes AT_A. */
int pq_kkt_batch_update_data_dense(pq_kkt_batch *k, const double *P_utri, const double *AT, const double *GT, int options, int mem);
/* dense/kkt.hpp:73-84, per instance, ONE launch for the batch: z_reg_inv = 1 / z_reg, the assembly straight into the LDS square, its factorisation.  delta[batch],
 * x_reg[batch][n], z_reg[batch][m].  Returns the number of instances that factored (negative = PQ_ERR_*), when the factors are complete. */
int pq_kkt_batch_update_scalings_and_factor(pq_kkt_batch *k, const double *delta, const double *x_reg, const double *z_reg, int mem);
/* of the last factorisation, per instance: ok_host[batch] = 1 / 0, first_bad_col_host[batch] (may be NULL) = -1 or the failing column (LLT: a pivot that is not
 * positive; LDLT: an exact zero only).  The stored factor of a failed instance is unspecified. */
int pq_kkt_batch_info(const pq_kkt_batch *k, int *ok_host, int *first_bad_col_host);
/* dense/kkt.hpp:86-105, per instance, one launch.  The lhs_* blocks of an instance whose last factorisation failed are left untouched.  Outputs must not overlap
 * inputs.  rhs_y / lhs_y (rhs_z / lhs_z) may be null when p == 0 (m == 0).  PQ_ERR_INVALID before the first factorisation. */
int pq_kkt_batch_solve(pq_kkt_batch *k, const double *rhs_x, const double *rhs_y, const double *rhs_z, double *lhs_x, double *lhs_y, double *lhs_z, int mem);
/* dense/kkt.hpp:108-132, per instance, one launch each.  With p == 0 (resp. m == 0) zn is not written and zt is all +0.0. */
int pq_kkt_batch_eval_P_x(pq_kkt_batch *k, const double *alpha, const double *x, double *z, int mem);
int pq_kkt_batch_eval_A_xn_and_AT_xt(pq_kkt_batch *k, const double *alpha_n, const double *alpha_t, const double *xn, const double *xt, double *zn, double *zt,
                                     int mem);
int pq_kkt_batch_eval_G_xn_and_GT_xt(pq_kkt_batch *k, const double *alpha_n, const double *alpha_t, const double *xn, const double *xt, double *zn, double *zt,
                                     int mem);
/* test hooks, out_host n x n column-major, lower triangle meaningful.  internal_kkt_mat RECOMPUTES the matrix of one instance from the stored data and the stored
 * scalings of the last factorisation (an assemble-only instantiation of the factorisation kernel's code: the hot path never writes the assembled matrix to memory);
 * internal_factor copies the stored factor. */
int pq_kkt_batch_internal_kkt_mat(pq_kkt_batch *k, int instance, double *out_host);
int pq_kkt_batch_internal_factor(pq_kkt_batch *k, int instance, double *out_host);
/* out3[0]: device time of the last factorisation launch, out3[1]: device time of the last solve launch (hipEvents), out3[2]: wall time of the last
 * pq_kkt_batch_update_scalings_and_factor call, all in ms */
int pq_kkt_batch_last_ms(const pq_kkt_batch *k, double out3[3]);

/* ===================== KKTSystem for a BATCH of small dense QPs (over the backend above) ===================== */
/* `batch` instances of piqp::KKTSystem (kkt_system.hpp) over the dense batch backend (csrc/dense_kktsys_batch.hip): per instance the scalings x_reg / z_reg, the
 * elimination of the slacks from a right-hand side, the backend solve with the iterative-refinement loop, the recovery of the ten-vector step and mul are those of
 * the CPU oracle (oracle/orc_kkt_system.c over oracle/orc_dense.c) bit for bit.  update_scalings_and_factor, solve and mul are ONE launch each; solve runs one
 * workgroup per instance, so every instance takes its own number of refinement steps and the host takes no part in the loop.
 * The instances share n <= PQ_KKT_BATCH_DENSE_MAX_N, p, m (not limited), the factorisation kind (settings->kkt_solver: PQ_DENSE_CHOLESKY or PQ_DENSE_LDLT_NO_PIVOT),
 * one pq_settings and the four finite-bound index lists (ascending, HOST memory in either mode; every row of G is in h_l_idx or h_u_idx).  x_b_scaling is per
 * instance, [batch][n]; NULL = all ones.  Matrices: the layout of pq_kkt_batch_create_dense.  mem (pq_mem) says where EVERY array argument of that call lives.
 * A batch of variables is a pq_vars whose ten pointers are [batch][len] arrays, len the single-instance length (n, p, m, m, n, n, m, m, n, n); of the box vectors
 * the first n_x_l / n_x_u entries of each row are meaningful, the rest is neither read nor written.  A pointer whose vector has no meaningful entry may be NULL. */
typedef struct pq_kktsys_batch pq_kktsys_batch;
/* Arguments are checked before the device is touched.  Refuses what pq_kkt_batch_create_dense refuses (PQ_ERR_UNSUPPORTED for n > PQ_KKT_BATCH_DENSE_MAX_N), and
 * with PQ_ERR_INVALID: a NULL settings, iterative_refinement_max_iter outside [0, 64] (a safety cap on the in-kernel loop), a negative count, a count above its
 * vector's length, a NULL list with a positive count, a list that is not strictly ascending or has an index out of range, a row of G in neither h_l_idx nor
 * h_u_idx.  Allocates everything the handle will ever need, host-mode staging included: pq_debug_alloc_count() moves in no later call except _clone / _clone_select. */
int pq_kktsys_batch_create_dense(pq_kktsys_batch **out, int device, int batch, int n, int p, int m, const double *P_utri, const double *AT, const double *GT,
                                 int n_h_l, int n_h_u, int n_x_l, int n_x_u, const int *h_l_idx, const int *h_u_idx, const int *x_l_idx, const int *x_u_idx,
                                 const double *x_b_scaling, const pq_settings *settings, int mem);
/* The same with finite-bound lists of its OWN for every instance.  counts: int [batch][4] = n_h_l, n_h_u, n_x_l, n_x_u per instance; the four list arrays are
 * int [batch][m], [batch][m], [batch][n], [batch][n], row i meaningful in its first counts[i][k] entries; all HOST memory in either mode.  Every check of the
 * creator above is made per instance before the device is touched, and the error text names the instance; a NULL counts is refused.  Of the box vectors of a
 * pq_vars the first counts[i][2] / counts[i][3] entries of row i are meaningful; a box pointer may be NULL only when no instance uses that vector.  On the device
 * the tables get one row of 2 m + 4 n ints per instance; a handle of the creator above keeps its one shared row and reads nothing per instance. */
int pq_kktsys_batch_create_dense_lists(pq_kktsys_batch **out, int device, int batch, int n, int p, int m, const double *P_utri, const double *AT, const double *GT,
                                       const int *counts, const int *h_l_idx, const int *h_u_idx, const int *x_l_idx, const int *x_u_idx,
                                       const double *x_b_scaling, const pq_settings *settings, int mem);
/* Replaces the lists of a handle of pq_kktsys_batch_create_dense_lists (arguments and checks as there; a failed check leaves the handle as it was).  Allocates
 * nothing.  The factors and the stored scalings belong to the old lists: solve, mul and state return PQ_ERR_INVALID until the next update_scalings_and_factor, as
 * before the first.  PQ_ERR_INVALID on a handle whose lists are shared. */
int pq_kktsys_batch_set_lists(pq_kktsys_batch *k, const int *counts, const int *h_l_idx, const int *h_u_idx, const int *x_l_idx, const int *x_u_idx);
void pq_kktsys_batch_destroy(pq_kktsys_batch *k);
int pq_kktsys_batch_clone(const pq_kktsys_batch *k, pq_kktsys_batch **out); /* kkt_system.hpp:70-95: the scalings state is copied, the backend cloned; so are the kind of the lists and the tables */
/* Clone by a list of instances, under the rules and refusals of pq_kkt_batch_clone_select, over a backend cloned by the same list: instance j of the new handle
 * is instance idx[j] of k in every state vector (the P_diag of the last update_data that carried P and x_b_scaling included), its refinement flag and the
 * diagnostics of its last solve; with lists per instance it takes that instance's row of the tables (2 m + 4 n ints) and its four counts, with shared lists the
 * one table is copied.  The settings are copied as they stand.  A clone taken after update_scalings_and_factor solves and multiplies without factoring. */
int pq_kktsys_batch_clone_select(const pq_kktsys_batch *k, const int *idx, int count, pq_kktsys_batch **out);
int pq_kktsys_batch_dims(const pq_kktsys_batch *k, int *batch, int *n, int *p, int *m);
pq_kkt_batch *pq_kktsys_batch_backend(pq_kktsys_batch *k); /* borrowed; NULL for a NULL handle */
/* kkt_system.hpp:134-141: pq_kkt_batch_update_data_dense on the backend; a non-NULL x_b_scaling is re-read */
int pq_kktsys_batch_update_data_dense(pq_kktsys_batch *k, const double *P_utri, const double *AT, const double *GT, const double *x_b_scaling, int options, int mem);
int pq_kktsys_batch_set_settings(pq_kktsys_batch *k, const pq_settings *settings); /* kkt_solver is not re-read */
/* kkt_system.hpp:143-211 per instance, ONE launch.  iterative_refinement: int [batch], NULL = off everywhere; rho, delta: double [batch].  Afterwards the borrowed
 * backend is in the state pq_kkt_batch_update_scalings_and_factor(delta_reg, x_reg, z_reg_iter_ref) would have left.  Returns the number of instances that
 * factored (negative = PQ_ERR_*). */
int pq_kktsys_batch_update_scalings_and_factor(pq_kktsys_batch *k, const int *iterative_refinement, const double *rho, const double *delta, const pq_vars *vars,
                                               int mem);
/* kkt_system.hpp:213-369 per instance, ONE launch, one workgroup per instance, the refinement loop (:256-301) inside it.  Returns the number of instances that
 * solved (negative = PQ_ERR_*).  The lhs blocks of an instance whose last factorisation failed are not touched; those of an instance that went non-finite are
 * unspecified.  Outputs must not overlap inputs.  PQ_ERR_INVALID before the first factorisation. */
int pq_kktsys_batch_solve(pq_kktsys_batch *k, const pq_vars *rhs, pq_vars *lhs, int mem);
/* kkt_system.hpp:392-425 per instance, one launch: rhs = K_full lhs with the scalings of the last update_scalings_and_factor */
int pq_kktsys_batch_mul(pq_kktsys_batch *k, const pq_vars *lhs, pq_vars *rhs, int mem);
/* of the last solve, host arrays [batch], any may be NULL: solve_ok 1 / 0 (0: a non-finite refine error, a non-finite lhs without refinement, a failed last
 * factorisation), refinement steps taken, backend solves of that solve, the last refine error and the norm of the condensed right-hand side (refinement only) */
int pq_kktsys_batch_info(const pq_kktsys_batch *k, int *solve_ok, int *refine_steps, int *backend_solves, double *refine_error, double *rhs_norm);
/* what: the condensed-system vectors the oracle keeps, copied to HOST memory [batch][len]: x_reg (n; includes the static regularisation), z_reg (m; without it),
 * rhs_x_bar (n), rhs_z_bar (m) of the last solve */
enum { PQ_KKTSYS_BATCH_X_REG = 0, PQ_KKTSYS_BATCH_Z_REG = 1, PQ_KKTSYS_BATCH_RHS_X_BAR = 2, PQ_KKTSYS_BATCH_RHS_Z_BAR = 3 };
int pq_kktsys_batch_state(pq_kktsys_batch *k, int what, double *out_host);
/* device time (hipEvents) of the last factor, solve and mul launch, ms */
int pq_kktsys_batch_last_ms(const pq_kktsys_batch *k, double out3[3]);

/* ===================== DenseSolver for a BATCH of small dense QPs (over the KKTSystem above) ===================== */
/* The device equivalent of
 *     for (i < batch) { DenseSolver s; s.settings() = settings; s.setup(P_i, c_i, A_i, b_i, G_i, h_l_i, h_u_i, x_l_i, x_u_i); s.solve(); }
 * (csrc/dense_solver_batch.hip): per instance status, iterations, trace, results and every non-time info field are those of the CPU oracle (oracle/orc_solver.c) bit
 * for bit.  n <= PQ_KKT_BATCH_DENSE_MAX_N; p and m are not limited; settings->kkt_solver is PQ_DENSE_CHOLESKY or PQ_DENSE_LDLT_NO_PIVOT.  The instances share n, p, m,
 * one pq_settings and, unless pq_solver_batch_set_bound_sets says otherwise, the set of finite bounds.  The solve runs in rounds clocked by the host: a small kernel advances every instance to its next KKTSystem call, then
 * the factor launch and the solve launch of pq_kktsys_batch_* run on the instances that asked for them; the host reads three counters per round.  The instances need
 * not run in lock step; an instance that has ended is not touched again.
 * pq_solver_batch_update_dense is DenseSolver::update (solver.hpp:218-308): per instance it un-scales everything stored, assigns what is
 * given, and scales again -- with the stored scalings when preconditioner_reuse_on_update is set or no matrix is given, else by a new equilibration -- so an update of
 * c alone moves P, A' and G' by roundings, as in the reference.  ONE RULE IS NOT THE REFERENCE'S: its dense backend recomputes A'A only when A is given
 * (dense/kkt.hpp:62-71); when P or G comes without A and the scalings are recomputed, A' is rescaled and A'A stays that of the old scalings, which turns solvable
 * problems into MAX_ITER_REACHED or PRIMAL_INFEASIBLE.  Here A'A is recomputed from the rescaled A' when A is given, or when any matrix is given and
 * preconditioner_reuse_on_update is 0; in every other case it is left alone, as the reference leaves it (the staleness is rounding only).  The state after such a call
 * is the reference's after update(..., A = its own unscaled A), bit for bit.
 * Every argument is checked before the device is touched: PQ_ERR_UNSUPPORTED for n > 128; PQ_ERR_INVALID for batch < 1, n < 1, negative p or m, another kkt_solver,
 * a NULL P or c, a NULL matrix with a positive count, iterative_refinement_max_iter outside [0, 64], a bad mem or order, a solve before a setup (status PQ_UNSOLVED)
 * and settings that verify_settings refuses (every instance PQ_INVALID_SETTINGS, no launch). */
typedef struct pq_solver_batch pq_solver_batch;
int pq_solver_batch_create(pq_solver_batch **out, int device);
void pq_solver_batch_destroy(pq_solver_batch *s);
pq_settings *pq_solver_batch_settings(pq_solver_batch *s); /* shared by all instances; kkt_solver and the preconditioner fields are read by setup */
/* A second handle in the state of s, without a new setup: the settings as they stand, the trace rows, the bound-set mode, solved / updated and the stored times
 * are copied, and the problem is cloned whole (_clone: the identity list) or by a list of instances (_clone_select: batch = count, instance j of the new handle is
 * instance idx[j] of s; idx in HOST memory, repeats allowed, count smaller or larger than the batch of s).  Per instance everything a later call can read goes
 * along bit for bit: the backend and the KKT system (pq_kktsys_batch_clone_select), the interior-point state, the results handed out, the info fields and the
 * trace, the scaled vectors, x_b_scaling, the preconditioner and, with PQ_BOUND_SETS_PER_INSTANCE, the instance's lists (tab has rows of 2 m + 2 n ints here) --
 * with shared sets the one table is copied.  So a clone taken after a solve answers info, get_result_mem and get_trace for its instances without solving, and an
 * update on it unscales with the stored scalings of its instances.  The new handle is on the same device with a stream of its own and is independent: it survives
 * pq_solver_batch_destroy(s), and no call on either is seen by the other; s is only waited for and read.  The call is the only one on the new handle that
 * allocates: update, solve and the getters after it leave pq_debug_alloc_count() where it is, as after a setup.
 * _clone of a handle that was never set up gives a handle with those scalars and no problem, and touches no device; _clone_select of one is PQ_ERR_INVALID, as
 * are, before the device is touched and with *out left alone: a NULL s, out or idx, count < 1, an idx[j] outside [0, batch) (the text names j and the value). */
int pq_solver_batch_clone(const pq_solver_batch *s, pq_solver_batch **out);
int pq_solver_batch_clone_select(const pq_solver_batch *s, const int *idx, int count, pq_solver_batch **out);
/* of the clone call that made s: out2 = { wall ms of the call from the upload of the list to the last wait, device ms of the gathers of the three layers (hipEvents
 * of the new handles around them; the memsets of a layer's fresh buffers that run between its events count) }; both 0 on a handle that pq_solver_batch_create made
 * or whose source was never set up.  Wall minus device is the allocation and the host images. */
int pq_solver_batch_clone_ms(const pq_solver_batch *s, double out2[2]);
/* Who owns the set of finite bounds.  PQ_BOUND_SETS_SHARED (the default): one set for the batch, a checked promise -- setup refuses an instance that differs from
 * instance 0 and update refuses a bound that turns infinite or finite, as described at those calls.  PQ_BOUND_SETS_PER_INSTANCE: every instance has the lists
 * DenseSolver would hold for its own vectors (dense/data.hpp:98-207), at setup and after every update, so constraints can be switched off per instance with
 * -/+ infinity and come back later.  The mode is read by setup; a problem that is set up keeps the mode its setup read.  PQ_ERR_INVALID for any other value and
 * for a NULL handle. */
enum { PQ_BOUND_SETS_SHARED = 0, PQ_BOUND_SETS_PER_INSTANCE = 1 };
int pq_solver_batch_set_bound_sets(pq_solver_batch *s, int mode);
/* DenseSolver::setup per instance.  P [batch] n x n, A [batch] p x n, G [batch] m x n: stacks of matrices in the layout `order` (PQ_COL_MAJOR / PQ_ROW_MAJOR) and
 * under the ordering contract of pq_solver_setup_dense_mem; vectors [batch][len]; NULL optionals as in the single solver.  mem: where EVERY array lives.  The
 * finite-bound pattern is taken from instance 0; another instance that differs is refused (PQ_ERR_INVALID, as pq_batch_update does) -- with
 * PQ_BOUND_SETS_PER_INSTANCE every instance gets its own lists, dropped rows and packed box vectors instead, and nothing is refused.  Rows of G without a finite bound
 * are zeroed (disable_inf_constraints), the Ruiz equilibration runs per instance (one kernel), and the internal pq_kktsys_batch is created on the scaled data.  May be
 * called again on the same handle; it is the only call besides create and destroy that may allocate.  Returns 1. */
int pq_solver_batch_setup_dense(pq_solver_batch *s, int batch, int n, int p, int m, const double *P, const double *c, const double *A, const double *b,
                                const double *G, const double *h_l, const double *h_u, const double *x_l, const double *x_u, int mem, int order);
/* DenseSolver::update per instance, on the device, where the data stand.  Any pointer may be NULL (unchanged); all NULL is an unscale and a rescale, as in the
 * reference.  Shapes, layouts, mem and order as in pq_solver_batch_setup_dense.  settings.preconditioner_reuse_on_update, preconditioner_iter and
 * preconditioner_scale_cost are read at the call.  The set of finite bounds stays the setup's: the lists the reference would hold after the call (set_h_l / set_h_u
 * with the given vector for a given side and the stored finiteness for the other, a row dropped at setup being stored finite on both sides as -1 / 1; then
 * disable_inf_constraints, set_x_l, set_x_u) are worked out on the host, and if those of any instance differ from the setup's the call returns PQ_ERR_INVALID and the
 * handle is as it was.  As in the reference, a row whose two bounds are both given infinite has its column of G' zeroed and its bounds set to -1 / 1, and the columns of
 * a new G' of rows dropped earlier are zeroed only in a call that also gives h_l or h_u.  PQ_ERR_INVALID before the device is touched: a NULL handle, a call before a
 * setup, a bad mem or order, A or b with p = 0, G, h_l or h_u with m = 0.  The call allocates nothing.  The next solve starts every instance from INIT (no warm start);
 * statuses, results and traces of the previous solve stay readable until then.  info.update_time is the wall time of the call (the batch's), and a solve after an
 * update reports run_time = update_time + solve_time.  Returns 1.
 * With PQ_BOUND_SETS_PER_INSTANCE the call never refuses on finiteness: the lists of every instance are worked out in the same way and REPLACE its own, in the tables
 * here and in the internal KKT system (pq_kktsys_batch_set_lists), and a given box vector is packed to its new list (a variable whose bound is no longer in the list
 * has no entry).  A row that comes back keeps the zero column of G' until a G is given, as in the reference.  Everything else above holds unchanged, A'A, rows
 * dropped earlier, no warm start and no allocation included.  A SECOND RULE IS NOT THE REFERENCE'S, and it can show in this mode only: a stored infinite bound is
 * infinite.  The reference stores it as -/+ 1e30, scales it with its row and un-scales it at the next update, and (1e30 d) (1 / d) may round to the neighbour of
 * 1e30, which disable_inf_constraints sees as finite.  So when h_l or h_u comes ALONE and is infinite on a row whose other side is stored infinite, the reference
 * either drops the row or, by the rounding of that product, leaves it in neither list -- a row without a bound, whose solves turn into NaN.  Here the row is
 * dropped.  With both vectors given, or with finite numbers on such rows, the lists are the reference's. */
int pq_solver_batch_update_dense(pq_solver_batch *s, const double *P, const double *c, const double *A, const double *b, const double *G, const double *h_l,
                                 const double *h_u, const double *x_l, const double *x_u, int mem, int order);
/* of the last update: out2 = { wall ms, device ms (hipEvents around its kernels and copies) } */
int pq_solver_batch_last_update_ms(const pq_solver_batch *s, double out2[2]);
/* solve() of every instance; returns the number of instances that ended PQ_SOLVED (>= 0).  The number of rounds is bounded before the loop starts by
 * (max_iter + 1) (max_factor_retires + 4); a loop that reaches the bound returns PQ_ERR_INTERNAL and leaves every unfinished instance PQ_UNSOLVED. */
int pq_solver_batch_solve(pq_solver_batch *s);
/* result().info of one instance, n_factor and n_solve included; update_time, solve_time and run_time are the batch's, the other time fields are 0 */
const pq_info *pq_solver_batch_info(const pq_solver_batch *s, int instance);
/* field 0..9 of Variables of ALL instances into a host or device array [batch][len], len as in the single solver's result (the box vectors at full length n,
 * restore_dual applied).  Device mode makes no allocation. */
int pq_solver_batch_get_result_mem(pq_solver_batch *s, int field, double *out, int mem);
/* ACTING ON A LIST OF INSTANCES, IN PLACE (the _select forms of pq_solver_batch_solve, pq_solver_batch_update_dense and pq_solver_batch_get_result_mem): the same
 * handle, the same buffers, the same result arrays -- no second handle as with pq_solver_batch_clone_select.  idx: `count` instances in HOST memory; the value arrays
 * and out are [count][...], row j belongs to instance idx[j]; mem and order mean what they mean in the whole-batch calls.
 * A LISTED instance ends in the state the whole-batch call would leave it in when given the same row, bit for bit: the ten result vectors, status, iter and every
 * non-time info field (n_factor, n_solve, n_backend_solve), every trace row and the row count, the 13 items of pq_solver_batch_scaled_data, its lists with
 * PQ_BOUND_SETS_PER_INSTANCE, and the state of the borrowed KKT system (pq_kktsys_batch_state, pq_kktsys_batch_info, pq_kkt_batch_internal_factor).  The same device
 * functions run on the same row: every launch is sized by the list, one workgroup per listed instance (in the packed factor kernel of n < 32 one wave), which
 * reads its instance from the list; the activity words of an instance that is not listed are never read.
 * Of an UNLISTED instance no observable byte changes: the results handed out, pq_info with its times, the trace, the scaled data and scalings, its bound lists, the
 * KKT system's state and factor.  No workgroup runs on it.  (Host images travel whole where the whole-batch calls move them whole -- the state records around a
 * solve, the bound tables of PQ_BOUND_SETS_PER_INSTANCE in an update: an unlisted row gets the bytes it holds.)
 * _solve_select: returns how many of the listed instances ended PQ_SOLVED.  The settings are read as they stand at the call (stragglers are run again in place
 * under a larger max_iter).  Every listed instance starts from INIT as in pq_solver_batch_solve (no warm start) and its trace at row 0.  The rounds end when every
 * listed instance is done; their bound is pq_solver_batch_solve's: when it is reached PQ_ERR_INTERNAL is returned and only the listed unfinished instances become
 * PQ_UNSOLVED.  Settings that verify_settings refuses: the listed infos alone become PQ_INVALID_SETTINGS, no launch, PQ_ERR_INVALID.  solve_time and run_time are
 * written to the listed infos only; run_time keeps the handle-wide rule of pq_solver_batch_solve -- updated (any update call since the setup) ? update_time :
 * setup_time, plus solve_time -- where update_time is that of the instance's OWN last update (0 if it never had one).  pq_solver_batch_last_ms reports this
 * call.  Afterwards pq_solver_batch_get_result_mem, _get_trace and _info work for the whole batch: an instance that was never solved reads zeros, the status its
 * setup left and 0 trace rows.
 * _update_dense_select: the sequence of pq_solver_batch_update_dense (bound lists on the host, unscale, assign, rescale or re-equilibrate, P_diag, A'A under the A'A
 * rule above, x_b_scaling into the KKT system) on the listed rows only.  Shared bound sets: the finiteness check runs over the `count` rows given; a mismatch is
 * refused with pq_solver_batch_update_dense's text, naming the instance (not j), and the handle stays as it was.  Sets per instance: the lists of the listed
 * instances are rebuilt and no others; the borrowed KKT system then refuses its solve, mul and state calls (as after pq_kktsys_batch_set_lists) until EVERY instance
 * whose lists were replaced has been solved again, by list or whole -- a solve of other instances does not end that.  All pointers NULL: an unscale and rescale of the listed rows.  update_time goes to the listed infos,
 * pq_solver_batch_last_update_ms reports this call.  An updated instance keeps the results, info and trace of its last solve until it is solved again.  Returns 1.
 * _get_result_select_mem: field 0..9 of the listed instances -> out [count][len] by one gather kernel per `batch` entries of the list; repeats are allowed and
 * count may exceed the batch; a field of length 0 writes nothing and returns PQ_OK; it needs a previous solve, as pq_solver_batch_get_result_mem does.
 * ALLOCATION: the first _select call on a handle allocates one device int buffer of `batch` entries for the list (setup and clone allocate nothing for it).  After
 * that _solve_select, _update_dense_select from host or device memory and the device-memory result allocate nothing (pq_debug_alloc_count does not move); a
 * host-memory result stages [count][len].
 * REFUSED with PQ_ERR_INVALID before any device call, the handle untouched, the text opening with the call's name and naming j and the value where there is one:
 * a NULL s, idx or out; count < 1; a bad mem, order or field; a handle that is not set up; an idx[j] outside [0, batch); -- _solve_select and
 * _update_dense_select only -- an instance listed twice (two workgroups on one instance would race); the refusals of pq_solver_batch_update_dense (A or b with
 * p = 0; G, h_l or h_u with m = 0); for the result: no solve yet. */
int pq_solver_batch_solve_select(pq_solver_batch *s, const int *idx, int count);
int pq_solver_batch_update_dense_select(pq_solver_batch *s, const int *idx, int count, const double *P, const double *c, const double *A, const double *b,
                                        const double *G, const double *h_l, const double *h_u, const double *x_l, const double *x_u, int mem, int order);
int pq_solver_batch_get_result_select_mem(pq_solver_batch *s, const int *idx, int count, int field, double *out, int mem);
/* the 11-column table of solver.hpp:590-602 per instance, kept in device memory during the solve.  set_trace: rows per instance, before the setup (which sizes the
 * buffer; afterwards only a smaller number is accepted); every solve starts at row 0.  get_trace: rows_out rows of 11 doubles to HOST memory (out_host may be NULL) */
int pq_solver_batch_set_trace(pq_solver_batch *s, int max_rows);
int pq_solver_batch_get_trace(pq_solver_batch *s, int instance, double *out_host, int *rows_out);
int pq_solver_batch_dims(const pq_solver_batch *s, int *batch, int *n, int *p, int *m);
/* of the last solve: out6 = { wall ms, device ms summed over its launches (hipEvents), rounds, launches, device ms of the factor launches, of the solve launches } */
int pq_solver_batch_last_ms(const pq_solver_batch *s, double out6[6]);
/* test hooks.  scaled_data: one item of one instance after setup, to HOST memory: the scaled P_utri (n x n), AT (n x p), GT (n x m), c, b, h_l, h_u, x_l, x_u (the box
 * bounds compressed to the lists of that instance: the entries past its count are unspecified), x_b_scaling, and delta (n + p + m), delta_b (n), c (1) of the preconditioner.  kktsys: the borrowed KKT system; after a solve it is
 * in the state the last factorisation and the last solve of each instance left. */
enum { PQ_SOLVER_BATCH_P_UTRI = 0, PQ_SOLVER_BATCH_AT, PQ_SOLVER_BATCH_GT, PQ_SOLVER_BATCH_C, PQ_SOLVER_BATCH_B, PQ_SOLVER_BATCH_H_L, PQ_SOLVER_BATCH_H_U,
       PQ_SOLVER_BATCH_X_L, PQ_SOLVER_BATCH_X_U, PQ_SOLVER_BATCH_X_B_SCALING, PQ_SOLVER_BATCH_PRECOND_DELTA, PQ_SOLVER_BATCH_PRECOND_DELTA_B, PQ_SOLVER_BATCH_PRECOND_C };
int pq_solver_batch_scaled_data(pq_solver_batch *s, int instance, int what, double *out_host);
pq_kktsys_batch *pq_solver_batch_kktsys(pq_solver_batch *s);

/* ===================== small utilities used by the measurement harness ===================== */
/* fp64 MFMA / HBM micro-benchmarks on `device` (used once by bench.py to report measured peaks) */
/* number of device / pinned-host allocations the library has made in this process.  Contract (the reference's tests assert allocation-free
 * factor / solve, fwd.hpp:44-52): the counter moves only inside *_create / *_clone / *_clone_select (pq_kkt_batch_, pq_kktsys_batch_ and pq_solver_batch_clone_select, pq_solver_batch_clone) /
 * *_setup / *_update_data / *_partition calls, never in
 * update_scalings_and_factor, solve, eval_*, mul or condensed_residual, in either pointer mode */
long long pq_debug_alloc_count(void);
/* host-only (no device needed): the ticket-ordered task list of the persistent dense factorisation for a T x T grid of 128 x 128 tiles (csrc/dense_kernels.hip
 * k_chol_persistent), five ints per task (kind, round, a, b, gate).
 * Returns the number of tasks (-1: T outside [3, 1024]).  tests/test_chol_plan.py replays the list on the CPU: every task only waits for EARLIER tickets. */
int pq_debug_chol_plan(int T, int *out5, int capacity_tasks);
/* host-only (no device needed): the host logic of dense/data.hpp:98-207 for ONE instance -- set_h_l, set_h_u, disable_inf_constraints, set_x_l, set_x_u -- the very
 * function pq_solver_batch_setup_dense and pq_solver_batch_update_dense call for every instance in both modes of the bound sets (csrc/dense_solver_batch.hip
 * dsb_bound_lists).  h_l, h_u [m], x_l, x_u [n]: any may be NULL.  fin_*: all NULL for a setup (a vector that is not given is infinite everywhere); for an update
 * the finiteness flags (int, [m], [m], [n], [n]) of the four vectors as stored: 1 = in the list, a row dropped earlier being stored finite on both sides as
 * -1 / 1; 0 = infinite; a vector that is not given keeps what is stored (a stored infinite bound IS infinite: the second rule at pq_solver_batch_update_dense).  Outputs, any but counts may be NULL: counts = n_h_l, n_h_u, n_x_l, n_x_u; the four ascending lists ([m], [m], [n], [n]); dead [m]:
 * 1 on the rows dropped in this call (both bounds infinite; in both lists, bounds -1 / 1; an update without h_l and h_u drops nothing); the vectors as stored: a
 * given h vector (every one in a setup) at full length, one that an update does not give on the rows dropped in this call only; a given box vector (every one in a
 * setup) packed to its list and followed by zeros, one that an update does not give untouched.  Returns PQ_OK. */
int pq_debug_bound_lists(int m, int n, const double *h_l, const double *h_u, const double *x_l, const double *x_u, const int *fin_h_l, const int *fin_h_u,
                         const int *fin_x_l, const int *fin_x_u, int counts[4], int *h_l_idx, int *h_u_idx, int *x_l_idx, int *x_u_idx, int *dead, double *h_l_out,
                         double *h_u_out, double *x_l_out, double *x_u_out);
/* host-only (no device needed): the launch plan of the SYRK behind the dense KKT assembly and A^T A (csrc/dense_kernels.hip launch_syrk) for an n x n result with
 * inner dimension kdim, with (the G' W G assembly) or without (A^T A) the split-K workspace: out = { T = ceil(n / 128), tiles of the lower triangle, 1 if the 16-wave
 * low-latency shape runs (kdim <= 256), 1 if the launch asks for the XCD-aware tile-order table (if its allocation fails the launch falls back to the triangular
 * block -> tile map: the hook allocates nothing and cannot tell), rem = tiles of the split-K tail (0: none), k_split = K slices per tail tile }.
 * Computed by the functions the launcher itself uses; without a visible device the plan is that of 256 CUs.  Returns 0, or < 0 for a null out, n <= 0, kdim < 0 or
 * n > 32767 * 128.  tests/test_syrk_plan.py pins it for the shapes of
 * tests/test_dense_assembly_gpu.py. */
int pq_debug_syrk_plan(int n, int kdim, int with_workspace, int out[6]);
/* testing aid: out[i] = sqrt(in[i]) computed on `device` as the reference-order dense factorisation computes its pivots (csrc/dense_exact.hip); host arrays.
 * PQ_DENSE_CHOLESKY_EXACT is bitwise the reference only if the device's fp64 square root is correctly rounded: tests/test_dense_exact_gpu.py checks it. */
int pq_debug_device_sqrt(int device, const double *in, double *out, long long count);
int pq_microbench_mfma_f64(int device, int iters, double *tflops_out);
int pq_microbench_hbm_copy(int device, size_t bytes, int iters, double *gbps_out);
/* read + write GB/s of the fp64 transpose kernel the device-mode setup / update use (csrc/ingest_kernels.hip) on a rows x cols matrix, counted like the copy above */
int pq_microbench_transpose(int device, int rows, int cols, int iters, double *gbps_out);
/* debugging aid: average microseconds of the 128 x 128 diagonal-block factorisation kernel and 64 in-kernel shader-clock stamps
 * (step k at stamps64[8 k + q], see potrf_block in csrc/dense_kernels.hip); stamps64 may be NULL */
int pq_microbench_potrf_block(int device, int ldlt, int reps, double *us_out, long long *stamps64);
/* testing aid: the diagonal-block factorisation kernel (potrf_block: the unblocked part of Eigen::LLT, dense/kkt.hpp:82, resp. dense/ldlt_no_pivot.hpp:278-311) on the
 * caller's symmetric block A of order nb <= 128 (host memory, column-major, leading dimension 128, lower triangle read), `reps` times.  Outputs of the last repetition
 * (host memory): the factor L (128 x 128, lower triangle; LDLT: unit L with D on the diagonal), the reciprocal pivots rdiag[128] (LLT: 1 / l_cc, LDLT: 1 / d_c), D dvec[128]
 * (LDLT), the operand pack of the panel solve pack[36 * 256] (blocks j (j - 1) / 2 + k: -L(j, k), blocks 28 + k: the inverse of L_kk; column-major 16 x 16 each), info
 * (-1 or the first failing column), and the number of repetitions whose outputs differ from the first one's in any bit (0: the kernel is deterministic) */
int pq_debug_potrf_block(int device, int ldlt, int nb, int reps, const double *A, double *L, double *rdiag, double *dvec, double *pack, int *info, int *differing_reps);
/* testing aid: ONE operation of the CSC mat-vec layer under every sparse backend (csrc/sparse_ops.hip, CscOperators) on the caller's data, with no symbolic analysis and
 * no factorisation: the operators are built from `data` (host arrays), the values are replaced through the update path when P_val2 / AT_val2 / GT_val2 are given (all
 * three then, same patterns; an array of a matrix without entries may be NULL), the operation runs once on a stream of its own in the default or (ref_order != 0) the
 * reference-order mode, and the results come back.  All vectors are HOST memory.  The three outputs out_x[n], out_y[p], out_z[m] are copied DOWN before the operation
 * and back up after it whatever the operation writes, so an entry it leaves alone keeps the caller's value.  A NULL input vector is read as zeros.
 *   PQ_CSC_EVAL_P_X:  out_x = alpha_n P in_x
 *   PQ_CSC_EVAL_A:    out_y = alpha_n A in_x, out_x = alpha_t A' in_y         PQ_CSC_EVAL_G: out_z = alpha_n G in_x, out_x = alpha_t G' in_z
 *   PQ_CSC_FOLD_RHS:  out_x = rhs_x + G' (zinv .* rhs_z) + delta_inv A' rhs_y  (with_A / with_G: 0 leaves the term out)
 *   PQ_CSC_RECOVER_DUALS: out_y = delta_inv A in_x - delta_inv rhs_y, out_z = (G in_x - rhs_z) .* zinv  (with_A / with_G: 0 leaves the output alone)
 *   PQ_CSC_FOLD_RHS_ROWS, PQ_CSC_RECOVER_DUALS_ROWS: the same two on the listed rows (rows_x[nx]; rows_y[ny], rows_z[nz])
 *   PQ_CSC_RESIDUAL_ROWS: the refinement residual of (in_x, in_y, in_z) against rhs_* with x_reg, delta, z_reg on the listed rows into out_*; absmax_bits receives the
 *                     bit pattern of max |err| over them (NaN-propagating, 0 for no rows) and result 1, or result 0 when a column is too long for this form
 *   PQ_CSC_P_DIAG:    out_x = diag(P) */
enum { PQ_CSC_EVAL_P_X = 0, PQ_CSC_EVAL_A, PQ_CSC_EVAL_G, PQ_CSC_FOLD_RHS, PQ_CSC_RECOVER_DUALS, PQ_CSC_FOLD_RHS_ROWS, PQ_CSC_RECOVER_DUALS_ROWS, PQ_CSC_RESIDUAL_ROWS,
       PQ_CSC_P_DIAG };
typedef struct {
    double alpha_n, alpha_t, delta, delta_inv;
    int with_A, with_G;
    const double *P_val2, *AT_val2, *GT_val2;
    const double *in_x, *in_y, *in_z;
    const double *rhs_x, *rhs_y, *rhs_z, *zinv, *x_reg, *z_reg;
    const int *rows_x, *rows_y, *rows_z;
    int nx, ny, nz;
    double *out_x, *out_y, *out_z;
    unsigned long long absmax_bits;
    int result;
} pq_csc_op_io;
int pq_debug_csc_ops(int device, const pq_sparse_data *data, int op, int ref_order, pq_csc_op_io *io);
/* testing aid: the device Ruiz equilibration ALONE (csrc/ruiz_kernels.hip) on the caller's host arrays -- no solver, no KKT backend, no symbolic analysis.  Every array
 * below is HOST memory, read before and written after the one run; production code runs unchanged in between.
 *   path PQ_RUIZ_SOLVER_DENSE / PQ_RUIZ_SOLVER_SPARSE: what Solver::setup / update do -- a HostData and a Ruiz from the arrays, a DeviceRuiz (dense: upload_dense; sparse:
 *     host-fed), then scale(reuse = mode == PQ_RUIZ_REUSE, scale_cost, max_iter) or unscale().  Dense: P (the n x n column-major P_utri; only i <= j is touched), AT
 *     (n x p), GT (n x m).  Sparse: the three CSC triples, P / AT / GT their values.  batch, threads, stride, the tail and the guards are not used.
 *   path PQ_RUIZ_KERNEL: what the batched solver does -- launch_ruiz_sparse without a grid workspace on `batch` instances of one pattern, `threads` per workgroup
 *     (a multiple of 64, <= 1024), on an arena the hook lays out: per instance `stride` doubles holding, in this order and each between two runs of PQ_RUIZ_GUARD
 *     sentinel doubles, P | AT | GT values, c, x_b_scaling, delta, delta_inv, delta_b, delta_b_inv, scratch (n) and the tail b (p), h_l, h_u (m), x_l (n_x_l), x_u
 *     (n_x_u); what is left of the stride is sentinel too, and so are PQ_RUIZ_GUARD doubles before the first and after the last instance and around c_scale[batch].
 *     Arrays are [batch][len], instance after instance.  A NULL tail pointer reaches the kernel as NULL.  stride must hold the layout.
 * mode: PQ_RUIZ_COMPUTE reads the matrices, c and x_b_scaling; PQ_RUIZ_REUSE / PQ_RUIZ_UNSCALE also delta, delta_inv, delta_b, delta_b_inv and c_scale (the cost scaling
 * c; its inverse is formed as the solver forms it).  Every one of these comes back as the device left it.  guards (PQ_RUIZ_KERNEL): every sentinel double of the
 * arena in address order, then those around c_scale; guards_cap is the caller's capacity, guards_len the number written.  launch: what was launched last -- the
 * kernel (PQ_RUIZ_LAUNCH_*), grid x, grid y (dense: the tile grid of P; 1 otherwise), threads per workgroup.
 * Patterns, index lists, sizes and the stride are checked before anything is launched. */
enum { PQ_RUIZ_SOLVER_DENSE = 0, PQ_RUIZ_SOLVER_SPARSE, PQ_RUIZ_KERNEL };
enum { PQ_RUIZ_COMPUTE = 0, PQ_RUIZ_REUSE, PQ_RUIZ_UNSCALE };
enum { PQ_RUIZ_LAUNCH_DENSE = 0, PQ_RUIZ_LAUNCH_ONE_WG, PQ_RUIZ_LAUNCH_GRID };
#define PQ_RUIZ_GUARD 8
#define PQ_RUIZ_SENTINEL_BITS 0x7FF8DEADBEEF5AFEull /* a quiet NaN of fixed payload */
typedef struct {
    int path, mode, n, p, m, scale_cost, max_iter;
    int batch, threads;
    long long stride;
    const int *P_colptr, *P_rowind, *AT_colptr, *AT_rowind, *GT_colptr, *GT_rowind;
    double *P, *AT, *GT, *c, *x_b_scaling;
    double *delta, *delta_inv, *delta_b, *delta_b_inv, *c_scale;
    double *b, *h_l, *h_u, *x_l, *x_u;
    const int *x_l_idx, *x_u_idx;
    int n_x_l, n_x_u;
    double *guards;
    long long guards_cap, guards_len;
    int launch[4];
} pq_ruiz_io;
int pq_debug_ruiz(int device, pq_ruiz_io *io);

#ifdef __cplusplus
}
#endif
#endif /* PIQP_AMD_H */
