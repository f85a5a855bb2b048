// piqp_amd/csrc/dense_kkt_batch_internal.hpp -- what stands behind a pq_kkt_batch handle (dense_kkt_batch.hip), for the one other file that writes it:
// dense_kktsys_batch.hip, whose factorisation launch leaves the factor store, the stored scalings and the status exactly as pq_kkt_batch_update_scalings_and_factor
// does.  The launch-shape helpers (kb_factor_lds_bytes, kb_solve_lds_bytes) are in dense_kkt_batch_device.hpp.
#pragma once

#include "common.hpp"
#include "dense_kkt_batch_device.hpp"

struct pq_kkt_batch {
    int device = 0, batch = 0, n = 0, p = 0, m = 0, kind = PQ_DENSE_CHOLESKY;
    bool computed = false;
    int n_ok = 0;
    pq::DBuf<double> Pu, AT, GT, ATA, fac, delta_s, x_reg_s, zinv_s, mat_d;
    pq::DBuf<double> stage_in, stage_out;  // host-mode calls: batch (n + p + m + 2) resp. batch (n + p + m) doubles
    pq::DBuf<int> status;                  // [0, batch): info, [batch, 2 batch): first bad column
    pq::HBuf<int> status_h;
    pq::HBuf<double> mat_h;  // n x n
    pq::Event ev[4];  // factor begin / end, solve begin / end
    bool timed[2] = {false, false};
    double wall_ms = 0.0;
    pq::Stream st;
};

// The two heavy launches of a pq_kktsys_batch (dense_kktsys_batch.hip) on their own, for dense_solver_batch.hip, which clocks them in rounds: every pointer is
// device memory, the launch goes on the handle's stream, nothing is read back and nothing waits.  active: null = every instance; else int [batch], an instance
// whose word is 0 is left out (it reads nothing, writes nothing, and in the n < 32 variant its wave still reaches every barrier of its workgroup).
namespace pq {
void ksb_launch_factor(pq_kktsys_batch* k, const int* flags, const double* rho, const double* delta, const pq_vars& v, const int* active);
void ksb_launch_solve(pq_kktsys_batch* k, const pq_vars& rhs, const pq_vars& lhs, const int* active);
hipStream_t ksb_stream(pq_kktsys_batch* k);
const int* ksb_factor_status(const pq_kktsys_batch* k);  // device, [batch]: 0 = the instance's last factorisation succeeded
const int* ksb_solve_info(const pq_kktsys_batch* k);     // device, [3][batch]: solve_ok, refine steps, backend solves of the instance's last solve
void ksb_refresh_host(pq_kktsys_batch* k);               // reads status and diagnostics back as the public calls do, marks the handles factored and solved; waits
}  // namespace pq
