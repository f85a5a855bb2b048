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
