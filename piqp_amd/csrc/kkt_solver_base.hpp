// piqp_amd/csrc/kkt_solver_base.hpp
// Host-side mirror of piqp::KKTSolverBase<T,I,MatrixType> (reference include/piqp/kkt_solver_base.hpp:20-44)
// for device-resident data: same seven operations, same argument meaning, same bool/void error
// convention.  All vector arguments are DEVICE pointers on the backend's stream; the C-ABI layer
// (capi.cpp) stages host vectors when the caller uses PQ_MEM_HOST.  Backends are owned by std::unique_ptr from the
// moment they exist: clone() and every make_*_kkt factory return one.
#pragma once

#include <memory>
#include <stdexcept>
#include <vector>

#include "common.hpp"

namespace pq {

class KKTSolverBase {
public:
    virtual ~KKTSolverBase() = default;

    // kkt_solver_base.hpp:28
    virtual std::unique_ptr<KKTSolverBase> clone() const = 0;
    // kkt_solver_base.hpp:30 -- `data` is the C-ABI descriptor (host or device arrays per data->mem)
    virtual void update_data_dense(const pq_dense_data* data, int options) { (void)data; (void)options; throw std::runtime_error("update_data: wrong matrix type"); }
    virtual void update_data_sparse(const pq_sparse_data* data, int options) { (void)data; (void)options; throw std::runtime_error("update_data: wrong matrix type"); }
    // kkt_solver_base.hpp:32 -- x_reg[n], z_reg[m] device pointers, consumed during the call
    virtual bool update_scalings_and_factor(double delta, const double* x_reg, const double* z_reg) = 0;
    // kkt_solver_base.hpp:34
    virtual void solve(const double* rhs_x, const double* rhs_y, const double* rhs_z, double* lhs_x, double* lhs_y, double* lhs_z) = 0;
    // kkt_solver_base.hpp:37,39,41
    virtual void eval_P_x(double alpha, const double* x, double* z) = 0;
    virtual void eval_A_xn_and_AT_xt(double alpha_n, double alpha_t, const double* xn, const double* xt, double* zn, double* zt) = 0;
    virtual void eval_G_xn_and_GT_xt(double alpha_n, double alpha_t, const double* xn, const double* xt, double* zn, double* zt) = 0;
    // kkt_solver_base.hpp:43
    virtual void print_info() {}

    // device-side extras the KKTSystem needs (the reference reads these straight out of `data`)
    virtual const double* P_diag_device() const = 0;  // diag(P) for the static regularisation (kkt_system.hpp:198)
    virtual int n() const = 0;
    virtual int p() const = 0;
    virtual int m() const = 0;
    virtual hipStream_t stream() const = 0;
    virtual int device() const = 0;
    // test hooks (dense/kkt.hpp:134): copy n*n doubles to host
    virtual void internal_kkt_mat(double* out_host) { (void)out_host; throw std::runtime_error("internal_kkt_mat: dense only"); }
    // dense backends: true = a factorisation fails exactly where the reference's CLASS fails (LDLTNoPivot: an exact zero pivot, ldlt_no_pivot.hpp:307), not where this
    // library's dense_ldlt_no_pivot BACKEND also gives up (a pivot that is not positive); used by the raw factorisation object (pq_dense_factor)
    // dense backends with p = m = 0: factor the symmetric matrix of which A (device memory, column-major, leading dimension lda) holds the upper or (from_lower) the
    // lower triangle -- straight into the factor buffer, no data copy, no assembly; solve() then works as after update_scalings_and_factor.  (pq_dense_factor)
    virtual bool factor_symmetric(const double* A_dev, int lda, bool from_lower) { (void)A_dev; (void)lda; (void)from_lower; throw std::runtime_error("factor_symmetric: dense only"); }
    virtual void set_class_failure_semantics(bool on) { (void)on; throw std::runtime_error("set_class_failure_semantics: dense only"); }
    virtual void internal_factor(double* out_host) { (void)out_host; throw std::runtime_error("internal_factor: dense only"); }
    // test hook: rows of (start, diag_size, off_diag_size) of the multistage backend (print_info, multistage_kkt.hpp:385-393)
    virtual void multistage_block_info(std::vector<int>& out) const { (void)out; throw std::runtime_error("block_info: sparse_multistage only"); }
    // test hook (read-only): where the multistage chain kernels keep their working set -- { engine (0 chain, 1 tree), factor_in_lds, li_in_lds, solve_in_lds,
    // asm_chunks, max_h, max_w, factor_lds_bytes } (MultistageKKT::plan_lds)
    virtual void multistage_plan(int out[8]) const { (void)out; throw std::runtime_error("multistage_plan: sparse_multistage only"); }
    // symbolic-analysis figures of the sparse backends for the roofline arithmetic: N, nnz(PKPt), nnz(L) below the
    // diagonal, supernodes, tree levels, workgroup subtrees, max front order, factorisation flops
    virtual void sparse_stats(double out[8]) const { (void)out; throw std::runtime_error("sparse_stats: sparse backends only"); }
    // pq_kkt_sparse_ordering: the fill-reducing ordering and the elimination order built on it (perm[new] = old); returns 0 = amd, 1 = nested dissection
    virtual int sparse_ordering(int* fill_perm, int* elim_perm) const { (void)fill_perm; (void)elim_perm; throw std::runtime_error("sparse_ordering: sparse backends only"); }
    // stage-partitioned execution over several processes (include/piqp_amd.h, pq_kkt_partition)
    virtual void partition(int rank, int world, long long sizes[3]) { (void)rank; (void)world; (void)sizes; throw std::runtime_error("partition: not supported by this backend"); }
    virtual void set_exchange(pq_exchange_fn fn, void* user, double* buf_factor, double* buf_forward, double* buf_gather)
    {
        (void)fn; (void)user; (void)buf_factor; (void)buf_forward; (void)buf_gather;
        throw std::runtime_error("set_exchange: not supported by this backend");
    }
    // native transport: the library issues the RCCL collectives itself on its stream (pq_kkt_set_comm_rccl)
    virtual void set_comm_rccl(const unsigned char* id128, int rank, int world) { (void)id128; (void)rank; (void)world; throw std::runtime_error("set_comm_rccl: not supported by this backend"); }
    // true: this backend computes in the reference's own order of operations (sparse_exact.hip); the solver front end then runs the interior-point loop that
    // keeps that order too (the host loop of solver.cpp, vectors summed left to right like the reference's Eigen expressions restated by the CPU oracle)
    virtual bool reference_order() const { return false; }
    // test hook of the reference-order engine (sparse_exact.hip, pq_kkt_exact_factor): item 0 nnz(L), 1 L_cols, 2 L_ind, 3 L_vals, 4 D, 5 D_inv, 6 values of P K P', 7 perm;
    // copies the item to host memory when out_host != nullptr and returns its length
    virtual long long exact_factor(int what, void* out_host) { (void)what; (void)out_host; throw std::runtime_error("exact_factor: reference-order sparse engine only"); }
    // test hook: smallest |pivot| of the last factorisation (sparse backends), read back through the host
    virtual double min_abs_pivot() { throw std::runtime_error("min_abs_pivot: sparse backends only"); }
    virtual void native_exchange_calls(int out[3]) const { out[0] = out[1] = out[2] = 0; }
    // SURVEY 8(e) row 2 (round 4): with a stage partition the refinement residual err = rhs - K lhs (kkt_system.hpp:507-536) is evaluated only on the rows this
    // rank's part of the next solve reads -- its own subtrees' rows, the shared top, and nothing else -- and ||err||_inf crosses the ranks in ONE all-reduce(max)
    // per refinement step (exchange which = 3 on the buffer registered with set_exchange_norm; the native transport owns its buffer).  false: not sharded here
    // (single GPU, another KKT mode, a column too long for the row kernels): the caller evaluates the residual on every row as before.  On success *norm holds
    // the global ||err||_inf (+inf stands for NaN) and err_* are valid on this rank's rows only.
    virtual void set_exchange_norm(double* buf_norm) { (void)buf_norm; throw std::runtime_error("set_exchange_norm: not supported by this backend"); }
    virtual bool refine_error_sharded(const double* lhs_x, const double* lhs_y, const double* lhs_z, const double* rhs_x, const double* rhs_y, const double* rhs_z, const double* x_reg,
                                      double delta, const double* z_reg, double* err_x, double* err_y, double* err_z, double* norm)
    {
        (void)lhs_x; (void)lhs_y; (void)lhs_z; (void)rhs_x; (void)rhs_y; (void)rhs_z; (void)x_reg; (void)delta; (void)z_reg; (void)err_x; (void)err_y; (void)err_z; (void)norm;
        return false;
    }
    virtual void sharded_calls(int out[2]) const { out[0] = out[1] = 0; }
    // Condensed backends under a stage partition (round 5): a backend solve whose right-hand side is the residual refine_error_sharded left behind folds it into
    // this rank's x rows only and recovers the eliminated multipliers on the constraint rows next to them only; the refined multipliers of the eliminated blocks
    // are then complete on their owner rank and cross the ranks ONCE per KKTSystem::solve -- this call, made by KKTSystem::solve after its refinement loop took at
    // least one step (one all-gather, exchange which = 2).  No-op for every other backend.
    virtual void finish_sharded_solve(double* lhs_y, double* lhs_z) { (void)lhs_y; (void)lhs_z; }
    // pq_kkt_sharded_solve_calls: [0] sharded residual evaluations, [1] rows of this rank's share of the residual (of n + p + m), [2] backend solves that folded /
    // recovered on this rank's rows only, [3] all-gathers of the eliminated multipliers, [4] x rows folded per such solve, [5] constraint rows recovered per such solve
    virtual void sharded_solve_calls(int out[6]) const { for (int i = 0; i < 6; ++i) out[i] = 0; }  // [0] sharded residual evaluations, [1] rows of this rank's share (of n + p + m)
    // pq_kkt_comm_info: transport (0 none, 1 callback, 2 native RCCL), and for the native one what ncclCommCount / ncclCommUserRank / ncclCommCuDevice report
    virtual void comm_info(int out[4]) const { out[0] = 0; out[1] = out[2] = out[3] = -1; }
    virtual void partition_info(int out[8]) const { (void)out; throw std::runtime_error("partition_info: not supported by this backend"); }
    // measurement hooks (hipEvent brackets on the backend's stream)
    virtual void set_profiling(int level) { (void)level; }
    virtual void get_profile(int stage, double* total_ms, int* count) { (void)stage; *total_ms = 0.0; *count = 0; }
};

std::unique_ptr<KKTSolverBase> make_dense_kkt(const pq_dense_data* data, int kkt_solver, int device);
std::unique_ptr<KKTSolverBase> make_dense_exact_kkt(const pq_dense_data* data, int device);  // dense_exact.hip: dense_cholesky in the reference's own order of operations, n <= 1024
inline bool dense_kkt_kind(int k) { return k == PQ_DENSE_CHOLESKY || k == PQ_DENSE_LDLT_NO_PIVOT || k == PQ_DENSE_CHOLESKY_EXACT; }
constexpr int DENSE_EXACT_MAX_N = 1024;
void debug_device_sqrt(const double* in_host, double* out_host, long long count, int device);  // dense_exact.hip (pq_debug_device_sqrt)
void debug_csc_ops(const pq_sparse_data* data, int op, bool ref_order, pq_csc_op_io* io, int device);  // sparse_ops.hip (pq_debug_csc_ops)
std::unique_ptr<KKTSolverBase> make_sparse_kkt(const pq_sparse_data* data, int kkt_solver, int device);
std::unique_ptr<KKTSolverBase> make_multistage_kkt(const pq_sparse_data* data, int device);
// sparse_kkt.hip: the supernodal multifrontal engine, any KKTMode.  adopt: a stream the engine runs on and owns from the moment this returns (if it throws, the caller still owns it)
std::unique_ptr<KKTSolverBase> make_multifrontal_kkt(const pq_sparse_data* data, int mode, int device, hipStream_t adopt = nullptr);
std::unique_ptr<KKTSolverBase> make_exact_sparse_kkt(const pq_sparse_data* data, int mode, int device, double max_flops = 0.0);  // sparse_exact.hip: any KKTMode in the reference's own elimination order
hipStream_t release_exact_sparse_stream(KKTSolverBase* exact);  // an engine of make_exact_sparse_kkt gives its (idle) stream away; all it can do afterwards is be destroyed

}  // namespace pq
