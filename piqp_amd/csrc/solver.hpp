// piqp_amd/csrc/solver.hpp -- host-side front end: piqp::DenseSolver / SparseSolver (reference solver.hpp)
// over the device-resident KKTSystem.  The interior-point loop is the CALLER of the hot path: it is
// restated here on the host so that iteration counts can be compared with the CPU path; every
// KKT factor / solve / mat-vec it issues goes to the GPU through pq::KKTSystem.
#pragma once

#include <memory>
#include <vector>

#include "kkt_system.hpp"
#include "ruiz_device.hpp"

namespace pq {

using Vec = std::vector<double>;
using IVec = std::vector<int>;

// compressed sparse column, int32 / fp64 (typedefs.hpp:53-54)
struct Csc {
    int rows = 0, cols = 0;
    IVec colptr, rowind;
    Vec val;
    int nnz() const { return colptr.empty() ? 0 : colptr[cols]; }
};

// dense::Data<T> (dense/data.hpp:22-208) and sparse::Data<T,I> (sparse/data.hpp:26-231) in one struct
struct HostData {
    bool sparse = false;
    int n = 0, p = 0, m = 0;
    Vec P_utri, AT, GT;  // dense, column-major (n x n, n x p, n x m)
    Csc sP_utri, sAT, sGT;
    // sparse: gather maps from the caller's CSC value arrays (P full or upper, A, G as given at setup, nnz_in entries each) to the stored order of sP_utri / sAT /
    // sGT: stored value t = caller value src*[t] (build_sparse_ingest_maps).  values_on_device: the stored values live in DeviceRuiz only, s*.val stay empty.
    IVec srcP, srcA, srcG;
    int nnz_in[3] = {0, 0, 0};
    bool values_on_device = false;
    Vec c, b, h_l, h_u, x_l, x_u, x_b_scaling;
    int n_h_l = 0, n_h_u = 0, n_x_l = 0, n_x_u = 0;
    IVec h_l_idx, h_u_idx, x_l_idx, x_u_idx;

    void resize_vectors();
    void set_h_l(const double* v);
    void set_h_u(const double* v);
    bool disable_inf_constraints(std::vector<int>* rows = nullptr);  // true if a row was disabled (its G row zeroed; the rows are appended to *rows)
    void set_x_l(const double* v);
    void set_x_u(const double* v);
    pq_dense_data dense_descriptor() const;
    pq_sparse_data sparse_descriptor() const;
};

// dense::RuizEquilibration / sparse::RuizEquilibration (dense/preconditioner.hpp, sparse/preconditioner.hpp)
struct Ruiz {
    int n = 0, p = 0, m = 0;
    double c = 1.0, c_inv = 1.0;
    Vec delta, delta_b, delta_inv, delta_b_inv;
    void init(const HostData& d);
    void scale_data(HostData& d, bool reuse_prev_scaling, bool scale_cost, int max_iter, double epsilon = 1e-3);
    void unscale_data(HostData& d);
    // the vector part of unscale_data / scale_data(reuse): updates that touch no matrix leave the scaled matrices alone
    void unscale_vectors(HostData& d) const;
    void scale_vectors(HostData& d) const;
    // b, h_l, h_u, x_l, x_u alone (the matrices, c and x_b_scaling are DeviceRuiz's)
    void scale_bounds(HostData& d) const;
    void unscale_bounds(HostData& d) const;
};

struct HostVars {
    Vec x, y, z_l, z_u, z_bl, z_bu, s_l, s_u, s_bl, s_bu;
    void resize(int n, int p, int m);
    Vec& field(int k);
    const Vec& field(int k) const { return const_cast<HostVars*>(this)->field(k); }
};

// the interior-point loop with device-resident vectors (device_ipm.hip); the default path of Solver::solve
class DeviceIpm {
public:
    DeviceIpm();
    ~DeviceIpm();
    void init(const HostData& d, const Ruiz& rz, hipStream_t st);
    void refresh_data(const HostData& d, const Ruiz& rz);  // after setup / update: scaled vectors, Ruiz scalings, finite-bound masks
    int solve(KKTSystem& kkt, const pq_settings& set, const Ruiz& rz, pq_info& info, double* trace, int trace_max, int* trace_rows);
    void download_result(HostVars& out);  // unscaled, expanded (unscale_results + restore_dual already applied)

private:
    struct Impl;
    std::unique_ptr<Impl> I;
};

// The problem data of ONE setup() / update() call, as the C entry points receive it.  `mem` says where the value arrays live -- the matrices and the six vectors;
// index arrays are host memory always.  nullptr = absent (setup) / unchanged (update); n, p, m are read at setup only.
struct ProblemArgs {
    bool sparse = false;
    int n = 0, p = 0, m = 0;
    int mem = PQ_MEM_HOST, layout = PQ_COL_MAJOR;             // layout: storage order of the dense P (n x n), A (p x n), G (m x n)
    const double *P = nullptr, *A = nullptr, *G = nullptr;    // dense: the matrices; sparse: the values of the three CSC triples, beside
    const int *Pp = nullptr, *Pi = nullptr, *Ap = nullptr, *Ai = nullptr, *Gp = nullptr, *Gi = nullptr;  // their column pointers and row indices
    const double *c = nullptr, *b = nullptr, *h_l = nullptr, *h_u = nullptr, *x_l = nullptr, *x_u = nullptr;
};

class Solver {
public:
    explicit Solver(int device);
    ~Solver();
    std::unique_ptr<Solver> clone() const;

    pq_settings& settings() { return m_settings; }
    // solver.hpp:151-216 and :218-308.  Device memory (a.mem = PQ_MEM_DEVICE) goes to DeviceRuiz by kernel (ingest_kernels.hip), never through HostData -- or, where
    // device_ingest() is false, comes to the host first.  update() before a setup() of the same kind prints "Solver not setup yet" and returns false.
    bool setup(const ProblemArgs& a);
    bool update(const ProblemArgs& a);
    static bool device_ingest();                              // false under PIQP_AMD_DEBUG=host_ruiz: the matrices are scaled on the host there
    const long long* last_ingest() const { return ingest_; }  // pq_solver_last_ingest
    int solve();  // solver.hpp:69-148
    const pq_info& info() const { return m_info; }
    const HostVars& result() const { return m_result; }
    const HostData* data() const { return m_data.get(); }
    void set_trace(double* buf, int max_rows) { trace_ = buf; trace_max_ = max_rows; trace_rows_ = 0; }
    int trace_rows() const { return trace_rows_; }
    int device() const { return device_; }
    KKTSolverBase* backend() { return m_kkt_system ? m_kkt_system->backend() : nullptr; }

private:
    int solve_impl();
    struct FetchedVectors;
    ProblemArgs arrive(const ProblemArgs& in, size_t n, size_t p, size_t m, const size_t mat_len[3], FetchedVectors& stage);
    bool update_vectors_only(const ProblemArgs& a, double t0);
    bool update_dense(const ProblemArgs& a, double t0);
    bool update_sparse(const ProblemArgs& a, double t0);
    bool finish_update(int options, double t0);
    bool kkt_factor();
    void kkt_solve(const HostVars& rhs, HostVars& lhs);
    void eval_P_x(double alpha, const Vec& x, Vec& z);
    void eval_A(double an, double at, const Vec& xn, const Vec& xt, Vec& zn, Vec& zt);
    void eval_G(double an, double at, const Vec& xn, const Vec& xt, Vec& zn, Vec& zt);
    double calculate_mu() const;
    void calculate_step(double& alpha_s, double& alpha_z) const;
    void update_residuals_nr();
    void update_residuals_r();
    double primal_res_of(const HostVars& v) const;
    double dual_res_of(const Vec& x) const;
    double primal_prox_inf() const;
    double dual_prox_inf() const;
    void unscale_results();
    void restore_dual();
    void make_kkt();
    void scale_problem(bool reuse);
    void unscale_problem();
    void release_dense_staging();
    void stage_alloc();
    void to_device(const HostVars& h, pq_vars& d);
    void from_device(const pq_vars& d, HostVars& h);

    int device_;
    pq_settings m_settings;
    pq_info m_info{};
    std::unique_ptr<HostData> m_data;
    Ruiz m_preconditioner;
    std::unique_ptr<DeviceRuiz> druiz_;  // device side of m_preconditioner; null only under PIQP_AMD_DEBUG=host_ruiz
    std::unique_ptr<KKTSystem> m_kkt_system;
    bool m_first_run = true, m_setup_done = false, m_enable_iterative_refinement = false;
    HostVars m_result, res_nr, res, step, prox_vars;

    // device staging: two Variables sets + three work vectors per size class
    std::vector<DBuf<double>> dev_in_, dev_out_;
    pq_vars din_{}, dout_{};
    DBuf<double> dxa_, dxb_, dxc_, dya_, dyb_, dza_, dzb_;
    std::unique_ptr<DeviceIpm> dipm_;  // null when PIQP_AMD_HOST_IPM=1
    double* trace_ = nullptr;
    int trace_max_ = 0, trace_rows_ = 0;
    long long ingest_[2] = {0, 0};  // matrix bytes of the last setup / update: across the host-device link, device to device
};

bool verify_settings(const pq_settings& s);  // settings.hpp:84-106

// HostData of a setup.  on_device (a.mem = PQ_MEM_DEVICE / values_on_device): the matrix values stay where they are -- the dense matrices only say which exist,
// the sparse patterns and gather maps are built as ever -- and the rows of G without a finite bound, which DeviceRuiz then has to zero, are appended to *zeroed_rows.
std::unique_ptr<HostData> make_dense_host_data(const ProblemArgs& a, IVec* zeroed_rows = nullptr);
std::unique_ptr<HostData> make_sparse_host_data(int n, int p, int m, const int* Pp, const int* Pi, const double* Px, const double* c, const int* Ap, const int* Ai,
                                                const double* Ax, const double* b, const int* Gp, const int* Gi, const double* Gx, const double* h_l, const double* h_u,
                                                const double* x_l, const double* x_u, bool values_on_device = false, IVec* zeroed_rows = nullptr);
// The stored order of a sparse problem, from the patterns alone (host-only; pq_debug_sparse_ingest_maps): the patterns of U = upper(P) -- per column the entries on
// or above the diagonal, rows ascending --, AT = A^T and GT = G^T -- in transposition order, the one the retranspose of Solver::update_sparse produces -- and the
// gather maps to them: stored entry t = the caller's entry srcP[t] / srcA[t] / srcG[t].  Absent matrix: null pattern, n x 0 transpose, empty map.
void build_sparse_ingest_maps(int n, int p, int m, const int* Pp, const int* Pi, const int* Ap, const int* Ai, const int* Gp, const int* Gi, Csc& U, Csc& AT, Csc& GT,
                              IVec& srcP, IVec& srcA, IVec& srcG);

}  // namespace pq
