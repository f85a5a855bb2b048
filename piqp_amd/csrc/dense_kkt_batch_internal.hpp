// piqp_amd/csrc/dense_kkt_batch_internal.hpp -- what stands behind a pq_kkt_batch handle (dense_kkt_batch.hip), and what the layers above it
// (dense_kktsys_batch.hip, dense_solver_batch.hip) share with it on the host: the host-mode staging and the refinement cap (the length table of pq_vars, vars_lens, is common.hpp's).  Only
// dense_kkt_batch.hip writes the handle's fields, with one exception named at ksb_data_rewritten below (the solver's update rewrites Pu, AT, GT in place);
// dense_kktsys_batch.hip, whose factorisation launch leaves the factor store, the stored scalings and the status
// exactly as pq_kkt_batch_update_scalings_and_factor does, reads them and ends with kb_factor_done.  The launch-shape helpers (kb_factor_lds_bytes,
// kb_solve_lds_bytes) are in dense_kkt_batch_device.hpp.
#pragma once

#include <chrono>
#include <cstdint>
#include <stdexcept>

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

// ---- clone by a list of instances, the three layers' one way: instance j of the new handle is instance host[j] of the source.  The public call of the layer that
// is asked checks the list (kb_check_select, before the device is touched) and uploads it ONCE (dev, `count` ints, complete when the layers below are called); each
// layer gathers its own per-instance buffers on the new handle's stream with kb_gather_rows, one launch per array, and its host images with kb_gather_host.
// kb_gather_timed closes a layer's gathers: it waits for the stream and adds the time between the two events to sel.gather_ms.
struct KbSelect {
    const int *host, *dev;
    int count;
    double* gather_ms;  // null, or where every layer adds the device time of its gathers (hipEvents of the new handle around them, read after its wait)
};
inline int kb_check_list(const char* who, const int* idx, int count)
{
    if (!idx) return fail(PQ_ERR_INVALID, "%s: clone_select: idx is null", who);
    if (count < 1) return fail(PQ_ERR_INVALID, "%s: clone_select: count = %d, count >= 1 wanted", who, count);
    return PQ_OK;
}
inline int kb_check_select(const char* who, int batch, const int* idx, int count)
{
    if (int rc = kb_check_list(who, idx, count)) return rc;
    for (int j = 0; j < count; ++j)
        if (idx[j] < 0 || idx[j] >= batch) return fail(PQ_ERR_INVALID, "%s: clone_select: idx[%d] = %d outside [0, %d)", who, j, idx[j], batch);
    return PQ_OK;
}
template <class W>
void kb_gather_launch(hipStream_t st, void* dst, const void* src, const int* idx_d, size_t count, size_t row_bytes)
{
    const size_t wpr = row_bytes / sizeof(W);
    const size_t work = wpr >= (size_t)KB_GATHER_THREADS ? count * ((wpr + KB_GATHER_CHUNK - 1) / KB_GATHER_CHUNK)
                                                         : (count + KB_GATHER_THREADS / wpr - 1) / (KB_GATHER_THREADS / wpr);
    const unsigned grid = (unsigned)(work < (size_t)KB_GATHER_MAX_GRID ? work : (size_t)KB_GATHER_MAX_GRID);
    k_kb_gather_rows<W><<<grid, KB_GATHER_THREADS, 0, st>>>((W*)dst, (const W*)src, idx_d, count, wpr);
    PQ_HIP(hipGetLastError());
}
// dst[j][0 .. row_bytes) = src[idx_d[j]][0 .. row_bytes) for j < count, device memory, on `st`.  An empty buffer launches nothing.  16-byte words when the row and
// both bases allow (an array that stands behind another one in its allocation, as the fields of a VarSet do, need not be aligned to more than its element), else 8,
// else 4.
inline void kb_gather_rows(hipStream_t st, void* dst, const void* src, const int* idx_d, size_t count, size_t row_bytes)
{
    if (!count || !row_bytes) return;
    const size_t a = row_bytes | (size_t)(uintptr_t)dst | (size_t)(uintptr_t)src;
    if (a % 16 == 0) kb_gather_launch<uint4>(st, dst, src, idx_d, count, row_bytes);
    else if (a % 8 == 0) kb_gather_launch<unsigned long long>(st, dst, src, idx_d, count, row_bytes);
    else if (a % 4 == 0) kb_gather_launch<unsigned>(st, dst, src, idx_d, count, row_bytes);
    else throw std::runtime_error("gather: a row that is no multiple of 4 bytes");
}
// the mirror: dst[idx_d[j]][0 .. row_bytes) = src[j][0 .. row_bytes) -- with same_row src[idx_d[j]] -- for j < count, the entries of idx_d distinct
template <class W>
void kb_scatter_launch(hipStream_t st, void* dst, const void* src, const int* idx_d, size_t count, size_t row_bytes, bool same_row)
{
    const size_t wpr = row_bytes / sizeof(W);
    const size_t work = wpr >= (size_t)KB_GATHER_THREADS ? count * ((wpr + KB_GATHER_CHUNK - 1) / KB_GATHER_CHUNK)
                                                         : (count + KB_GATHER_THREADS / wpr - 1) / (KB_GATHER_THREADS / wpr);
    const unsigned grid = (unsigned)(work < (size_t)KB_GATHER_MAX_GRID ? work : (size_t)KB_GATHER_MAX_GRID);
    k_kb_scatter_rows<W><<<grid, KB_GATHER_THREADS, 0, st>>>((W*)dst, (const W*)src, idx_d, count, wpr, same_row ? 1 : 0);
    PQ_HIP(hipGetLastError());
}
inline void kb_scatter_rows(hipStream_t st, void* dst, const void* src, const int* idx_d, size_t count, size_t row_bytes, bool same_row = false)
{
    if (!count || !row_bytes) return;
    const size_t a = row_bytes | (size_t)(uintptr_t)dst | (size_t)(uintptr_t)src;
    if (a % 16 == 0) kb_scatter_launch<uint4>(st, dst, src, idx_d, count, row_bytes, same_row);
    else if (a % 8 == 0) kb_scatter_launch<unsigned long long>(st, dst, src, idx_d, count, row_bytes, same_row);
    else if (a % 4 == 0) kb_scatter_launch<unsigned>(st, dst, src, idx_d, count, row_bytes, same_row);
    else throw std::runtime_error("scatter: a row that is no multiple of 4 bytes");
}
template <class T>
void kb_gather_host(T* dst, const T* src, const int* idx, int count, size_t len)
{
    for (int j = 0; j < count && len; ++j) std::memcpy(dst + (size_t)j * len, src + (size_t)idx[j] * len, sizeof(T) * len);
}
inline void kb_gather_timed(const KbSelect& sel, hipStream_t st, hipEvent_t begin, hipEvent_t end)
{
    stream_wait(st);
    if (!sel.gather_ms) return;
    float ms = 0.f;
    PQ_HIP(hipEventElapsedTime(&ms, begin, end));
    *sel.gather_ms += ms;
}
// the layers below the one that was asked: a new handle that the caller owns from here on; they throw (nothing is left behind: the parts are held by their owners)
pq_kkt_batch* kb_clone_rows(const pq_kkt_batch* k, const KbSelect& sel);
pq_kktsys_batch* ksb_clone_rows(const pq_kktsys_batch* k, const KbSelect& sel);

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
// list, count: null and the batch = every instance, slot s of the grid is instance s (the code of before).  Else `count` distinct instances in device memory: the
// grid is sized by count and slot s works on instance list[s]; every array, `active` included, stays indexed by INSTANCE, and the words of an instance that is not
// listed are not read (they are stale from earlier solves).
void ksb_launch_factor(pq_kktsys_batch* k, const int* flags, const double* rho, const double* delta, const pq_vars& v, const int* active, const int* list, int count);
void ksb_launch_solve(pq_kktsys_batch* k, const pq_vars& rhs, const pq_vars& lhs, const int* active, const int* list, int count);
// After pq_kktsys_batch_set_lists the system is `stale` (its solve, mul and state calls are refused) until a factorisation.  A factor launch over the whole batch ends
// that; one over a list does not, because an instance outside the list may still hold a factor of its old lists.  The caller that launches by list keeps count and
// says here when every instance whose lists were replaced has been factored since.
void ksb_lists_factored(pq_kktsys_batch* k);
// The one writer of the backend's data outside dense_kkt_batch.hip: pq_solver_batch_update_dense (dense_solver_batch.hip) unscales, assigns and rescales Pu, AT and
// GT where they stand, by kernels on the handle's stream, and then says so here.  options: the PQ_KKT_UPDATE_* flags of the matrices its caller gave (P: the
// system's P_diag is taken again, as KKTSystem::update_data does); refresh_ata: A'A is computed again from AT (kb_refresh_ata, dense_kkt_batch.hip);
// x_b_scaling: device, [batch][n], copied into the system's own.  Everything goes on the stream, nothing waits.  list, count as above: with a list P_diag, A'A
// and the rows of x_b_scaling of the listed instances alone are taken again, each by a launch sized by count.
void ksb_data_rewritten(pq_kktsys_batch* k, int options, bool refresh_ata, const double* x_b_scaling, const int* list, int count);
void kb_refresh_ata(pq_kkt_batch* k, const int* list, int count);
hipStream_t ksb_stream(pq_kktsys_batch* k);
const int* ksb_factor_status(const pq_kktsys_batch* k);  // device, [batch]: 0 = the instance's last factorisation succeeded
const int* ksb_solve_info(const pq_kktsys_batch* k);     // device, [3][batch]: solve_ok, refine steps, backend solves of the instance's last solve
void ksb_refresh_host(pq_kktsys_batch* k);               // reads status and diagnostics back as the public calls do, marks the handles factored and solved; waits
}  // namespace pq
