// piqp_amd/csrc/ruiz_device.hpp -- Ruiz equilibration on the device (dense/preconditioner.hpp:62-258, sparse/preconditioner.hpp:65-290).
//
// Two shapes of the same arithmetic:
//   * sparse, batched: ONE workgroup per problem instance walks the shared CSC patterns; used by the batched solver (thousands of small
//     instances in one launch) and by the sparse Solver (one instance, one wide workgroup);
//   * dense: tiled multi-workgroup kernels over the column-major P_utri / AT / GT that stay resident in HBM (the dense Solver hands the
//     scaled device copies to the KKT backend; no scaled host mirror exists).
// Both reproduce the host routine Ruiz::scale_data of solver.cpp bit for bit: column / row inf-norms are max-reductions (exact in any order,
// done with integer atomic max on the bit patterns of the non-negative values), every product is applied in the host's order, the one sum
// (the cost scaling's mean column norm) is accumulated sequentially by one lane.
#pragma once

#include <memory>

#include "common.hpp"

namespace pq {

enum RuizMode { RUIZ_COMPUTE = 0, RUIZ_REUSE = 1, RUIZ_UNSCALE = 2 };

struct RuizSparseArgs {
    int n = 0, p = 0, m = 0;
    const int *Pp = nullptr, *Pi = nullptr, *ATp = nullptr, *ATi = nullptr, *GTp = nullptr, *GTi = nullptr;  // device patterns: P upper (n x n), AT (n x p), GT (n x m)
    long long stride = 0;                                                                                  // doubles between consecutive instances, every pointer below
    double *Px = nullptr, *ATx = nullptr, *GTx = nullptr, *c = nullptr, *xbs = nullptr;                    // scaled in place
    double *delta = nullptr, *delta_inv = nullptr, *delta_b = nullptr, *delta_b_inv = nullptr;             // n + p + m, n + p + m, n, n
    double* tmp = nullptr;                                                                                 // n doubles of scratch
    double *b = nullptr, *h_l = nullptr, *h_u = nullptr, *x_l = nullptr, *x_u = nullptr;                   // optional tail (preconditioner.hpp:208-221); x_l / x_u compressed
    const int *x_l_idx = nullptr, *x_u_idx = nullptr;
    int n_x_l = 0, n_x_u = 0;
    // box lists per instance instead (the batched solver with PQ_BOUND_SETS_PER_INSTANCE): row i of `lists` has n_x_l, n_x_u in its ints 2 and 3 and the two index
    // lists at the offsets lists_x_l / lists_x_u; null: the shared lists above
    const int* lists = nullptr;
    long long lists_stride = 0, lists_x_l = 0, lists_x_u = 0;
    double* c_scale = nullptr;  // [batch], not strided: the cost scaling c of every instance (out for RUIZ_COMPUTE, in otherwise)
    // one-workgroup-per-instance launches only: workgroup r equilibrates instance inst_list[r] -- its stride offset, its row of `lists`, its c_scale -- of a larger
    // arena (`batch` of launch_ruiz_sparse is then the length of the list); null: the identity
    const int* inst_list = nullptr;
    int mode = RUIZ_COMPUTE, scale_cost = 0, max_iter = 10;
    double eps = 1e-3;
    unsigned long long* grid_ws = nullptr;  // optional, ruiz_grid_ws_words() words: with it a single instance (batch == 1) is equilibrated by a grid of workgroups
};
void launch_ruiz_sparse(const RuizSparseArgs& a, int batch, int threads, hipStream_t s);
size_t ruiz_grid_ws_words();
struct RuizLaunch { int kernel = -1, gx = 0, gy = 0, threads = 0; };  // PQ_RUIZ_LAUNCH_*, grid, workgroup size
RuizLaunch ruiz_last_launch();                                        // of this thread's last launch_ruiz_sparse / DeviceRuiz run (test hook)
void debug_ruiz(pq_ruiz_io* io, int device);                          // pq_debug_ruiz

struct HostData;
struct Ruiz;

// Device side of the preconditioner of ONE Solver.  Dense problems: owns the (scaled) device matrices.  Sparse problems: owns device copies
// of the patterns and the value arrays.  A host-fed sparse solver uses them as staging: the values go up from and return to the host mirror (HostData::s*.val)
// around every run.  A device-fed one (HostData::values_on_device) keeps no mirror: the value arrays here are the solver's data, filled by ingest_sparse and
// handed to the KKT backend through sparse_descriptor.
class DeviceRuiz {
public:
    DeviceRuiz(int device, const HostData& d);
    ~DeviceRuiz();
    DeviceRuiz(const DeviceRuiz&) = delete;
    DeviceRuiz& operator=(const DeviceRuiz&) = delete;
    std::unique_ptr<DeviceRuiz> clone() const;

    // dense: (re)load the unscaled matrices named by `options` (PQ_KKT_UPDATE_*) from the host staging copies in d
    void upload_dense(const HostData& d, int options);
    // dense: the same from the caller's DEVICE arrays P (n x n), A (p x n), G (m x n) in storage order `layout` (PQ_COL_MAJOR: transpose kernel for A and G, masked
    // copy for P; PQ_ROW_MAJOR: plain copies of A and G, masked transpose for P).  The sources are only read; returns the bytes written.
    long long ingest_dense(const double* P, const double* A, const double* G, int layout, int options);
    // rows of G disabled by data.hpp:144-169 after the upload / ingest (sparse: only where the values live here, HostData::values_on_device)
    void zero_G_rows(const std::vector<int>& rows);
    // sparse, values_on_device: the value arrays named by `options` from the caller's DEVICE arrays in the CSC order given at setup, through the gather maps of
    // d (HostData::srcP / srcA / srcG; ingest_kernels.hip).  The sources are only read; returns the bytes written.
    long long ingest_sparse(const HostData& d, const double* Px, const double* Ax, const double* Gx, int options);
    void copy_values_from(const DeviceRuiz& o);               // sparse: the three value arrays of another instance of the same problem (Solver::clone)
    pq_sparse_data sparse_descriptor(const HostData& d) const;  // device-resident values + x_b_scaling, host index arrays (pq_sparse_data.mem = PQ_MEM_DEVICE)
    // scale_data / unscale_data of the matrices, c and x_b_scaling; the scalings land in rz, c / x_b_scaling in d (sparse: the matrix values too)
    void scale(HostData& d, Ruiz& rz, bool reuse_prev_scaling, bool scale_cost, int max_iter, double eps = 1e-3);
    void unscale(HostData& d, Ruiz& rz);
    pq_dense_data dense_descriptor(const HostData& d) const;  // device-resident matrices + host index lists

private:
    void run(HostData& d, Ruiz& rz, int mode, bool scale_cost, int max_iter, double eps);
    struct Impl;
    std::unique_ptr<Impl> I;
};

}  // namespace pq
