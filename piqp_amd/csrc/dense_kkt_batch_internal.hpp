// piqp_amd/csrc/dense_kkt_batch_internal.hpp -- what stands behind a pq_kkt_batch handle (dense_kkt_batch.hip), and what the layers above it
// (dense_kktsys_batch.hip, dense_solver_batch.hip) share with it on the host: the host-mode staging and the refinement cap (the length table of pq_vars, vars_lens, is common.hpp's).  Only
// dense_kkt_batch.hip writes the handle's fields, with one exception named at ksb_data_rewritten below (the solver's update rewrites Pu, AT, GT in place);
// dense_kktsys_batch.hip, whose factorisation launch leaves the factor store, the stored scalings and the status
// exactly as pq_kkt_batch_update_scalings_and_factor does, reads them and ends with kb_factor_done.  The launch-shape helpers (kb_factor_lds_bytes,
// kb_solve_lds_bytes) are in dense_kkt_batch_device.hpp.
#pragma once

#include <chrono>

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

namespace pq {

constexpr int KB_MAX_REFINE_ITER = 64;  // safety cap on the in-kernel refinement loop (the reference's default is 10)

// ---- host-mode staging: `stage` is device memory of the handle, `off` the next free place in it (advanced)
inline bool kb_bad_mem(int mem) { return mem != PQ_MEM_HOST && mem != PQ_MEM_DEVICE; }

// an input of `count` elements: the caller's device pointer, or its copy in the input staging (nothing to copy: the staging's base)
template <class T>
const T* kb_in(const DBuf<T>& stage, hipStream_t st, const T* src, size_t count, int mem, size_t& off)
{
    if (mem == PQ_MEM_DEVICE || count == 0) return mem == PQ_MEM_DEVICE ? src : stage.p;
    T* dst = stage.p + off;
    PQ_HIP(hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyHostToDevice, st));
    off += count;
    return dst;
}

// an output of `count` doubles: the caller's device pointer, or a place in the output staging (preload: the host's present values go there first, for the blocks
// a kernel leaves alone)
inline double* kb_out(const DBuf<double>& stage, hipStream_t st, double* dst, size_t count, int mem, size_t& off, bool preload)
{
    if (mem == PQ_MEM_DEVICE || count == 0) return mem == PQ_MEM_DEVICE ? dst : stage.p;
    double* d = stage.p + off;
    if (preload) PQ_HIP(hipMemcpyAsync(d, dst, sizeof(double) * count, hipMemcpyHostToDevice, st));
    off += count;
    return d;
}

inline void kb_back(hipStream_t st, double* host, const double* dev, size_t count, int mem)
{
    if (mem != PQ_MEM_DEVICE && count) PQ_HIP(hipMemcpyAsync(host, dev, sizeof(double) * count, hipMemcpyDeviceToHost, st));
}

// ---- the end of every factorisation launch on k->st (dense_kkt_batch.hip): the status is read back, then `n_more` further read-backs of the caller ride on the same
// wait, the stream is WAITED for, and the host side of the handle is left factored (computed, n_ok).  w0: when the call that the handle's events ev[0], ev[1] time
// began (timed[0], wall_ms), or null for a launch they do not time.  Returns the number of instances that factored.
struct KbReadback {
    void* host;
    const void* dev;
    size_t bytes;
};
int kb_factor_done(pq_kkt_batch* k, const std::chrono::steady_clock::time_point* w0, const KbReadback* more = nullptr, int n_more = 0);

// The two heavy launches of a pq_kktsys_batch (dense_kktsys_batch.hip) on their own, for dense_solver_batch.hip, which clocks them in rounds: every pointer is
// device memory, the launch goes on the handle's stream, nothing is read back and nothing waits.  active: null = every instance; else int [batch], an instance
// whose word is 0 is left out (it reads nothing, writes nothing, and in the n < 32 variant its wave still reaches every barrier of its workgroup).
void ksb_launch_factor(pq_kktsys_batch* k, const int* flags, const double* rho, const double* delta, const pq_vars& v, const int* active);
void ksb_launch_solve(pq_kktsys_batch* k, const pq_vars& rhs, const pq_vars& lhs, const int* active);
// The one writer of the backend's data outside dense_kkt_batch.hip: pq_solver_batch_update_dense (dense_solver_batch.hip) unscales, assigns and rescales Pu, AT and
// GT where they stand, by kernels on the handle's stream, and then says so here.  options: the PQ_KKT_UPDATE_* flags of the matrices its caller gave (P: the
// system's P_diag is taken again, as KKTSystem::update_data does); refresh_ata: A'A is computed again from AT (kb_refresh_ata, dense_kkt_batch.hip);
// x_b_scaling: device, [batch][n], copied into the system's own.  Everything goes on the stream, nothing waits.
void ksb_data_rewritten(pq_kktsys_batch* k, int options, bool refresh_ata, const double* x_b_scaling);
void kb_refresh_ata(pq_kkt_batch* k);
hipStream_t ksb_stream(pq_kktsys_batch* k);
const int* ksb_factor_status(const pq_kktsys_batch* k);  // device, [batch]: 0 = the instance's last factorisation succeeded
const int* ksb_solve_info(const pq_kktsys_batch* k);     // device, [3][batch]: solve_ok, refine steps, backend solves of the instance's last solve
void ksb_refresh_host(pq_kktsys_batch* k);               // reads status and diagnostics back as the public calls do, marks the handles factored and solved; waits
}  // namespace pq
