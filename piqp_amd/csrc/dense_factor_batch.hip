// piqp_amd/csrc/dense_factor_batch.hip -- pq_dense_factor_batch_*: Eigen::LLT and piqp::dense::LDLTNoPivot for a BATCH of small matrices (n <= 128), every matrix
// factored in the REFERENCE'S OWN ORDER of floating-point operations by one workgroup (n >= 32) or one wave (n < 32) with the matrix resident in LDS.
//
// Per matrix the factor, the status and every solve are those of the CPU oracle (oracle/orc_dense.c as oracle/Makefile builds it: -ffp-contract=fast, so its
// multiply-adds are fused) bit for bit.  This file is compiled with -ffp-contract=off (piqp_amd/build.py, NO_CONTRACT): every fused operation below is an explicit
// fma(), everything else rounds on its own.  Each element is one sequential chain and elements are independent, so the parallelism is across elements (and across
// the batch); no matrix instruction is used.  dense_exact.hip replays orc_llt_compute across workgroups (left-looking, one launch per panel); here one workgroup
// owns the whole matrix, so the replay is right-looking like the oracle itself, block by block, with workgroup barriers between the phases.
//
//   oracle (orc_dense.c)                      here (k_dfb_factor -> dfb_factor_in_lds, dense_factor_batch_device.hpp; L(i, j) is the LDS copy, column-major, leading dimension n | 1)
//   llt_unblocked                             column c of the diagonal block, thread t owns row k + t: the pivot thread  s = 0, s = fma(v, v, s) for ascending j,
//                                             x = a_cc - s (skipped for the block's first column), fail on !(x > 0), sqrt;  every row below  dst = fma(-L(i, j), L(c, j), dst)
//                                             for ascending j, after the barrier dst / x
//   ldlt_unblocked                            the same shape:  temp_j = L(j, j) * L(c, j) (a plain product),  s = fma(L(c, j), temp_j, s),  a_cc - s,  fail on x == 0.0 only;
//                                             rows below  dst = fma(-L(i, j), temp_j, dst),  dst / x
//   trsm_right_lower_trans                    one thread per row of A21:  x_j = fma(-x_kk, l_jkk, x_j) for ascending kk;  LLT then x_j / l_jj
//   orc_ldlt_no_pivot_compute :541-552        the same thread, after all columns of its row:  dinv = 1.0 / d_j,  col = x_j * dinv,  t = col * d_j -- t goes to the
//                                             UPPER triangle of the LDS square (the A21_tmp of ldlt_no_pivot.hpp:338 lives there too)
//   syrk_like_lower / micro_kernel            per element of the trailing lower triangle  acc = 0,  acc = fma(a_ikk, 0.0 + b_jkk, acc) over the block's columns ascending
//                                             (at most 16: one K block),  C = C - acc;  a = A21 (LLT) or t (LDLT), b = A21
//   orc_llt_solve_inplace /                   k_dfb_solve, one thread per right-hand side: the column-oriented forward sweep  x_i = fma(-l_ij, x_j, x_i);  the backward
//   orc_ldlt_no_pivot_solve_inplace           sweep's dot products run over contiguous memory, which the oracle's compiler vectorises as an in-order reduction: the
//                                             products are rounded on their own and subtracted in ascending order, only the last element of an odd count is a fused
//                                             multiply-add (ex_dot in dense_exact.hip states the same rule);  LLT divides by l_jj, the LDLT diagonal step is a division
//
// Launch shape.  The grid is the batch; a launch wider than the chip queues.  No workgroup waits for another: each reads its own matrices and writes its own factors,
// status words and failing columns.  n >= 32: 256 threads per matrix.  n < 32: four matrices per workgroup, one wave each; the last workgroup of a batch that is not
// a multiple of four runs partly empty (its idle waves only keep the barriers company).  A matrix that fails stops working; the barriers are reached by the whole
// workgroup all the same (n >= 32: the workgroup leaves the loops together; n < 32: the wave goes on with its work switched off).
// LDS: the full square per matrix with leading dimension n | 1 (odd), 129 x 128 doubles = 129 KiB at n = 128: a walk along a row then has an odd stride in doubles, so
// the lanes of a half-wave fall on different bank pairs, and a walk down a column is contiguous.
#include <chrono>
#include <cmath>
#include <memory>

#include "common.hpp"
#include "dense_factor_batch_device.hpp"

namespace pq {

namespace {

constexpr int DFB_SOLVE_THREADS = 64;
constexpr int DFB_NCH = 16;  // right-hand sides per workgroup of the solve

// KIND 0: Eigen::LLT, 1: LDLTNoPivot.  G: threads per matrix (256: one matrix per workgroup, 64: four).  width: n below 32 (unblocked), block_size_rule(n) above.
// upper != 0: the matrix is read from -- and the factor written to -- the upper triangle, transposed on the way (ldlt_no_pivot.hpp:357-371: the Lower code on the
// transposed view).  F: n x n per matrix, leading dimension n; only the named triangle is written, and only on success.  info: 0 / 1; badcol: -1 or the column.
template <int KIND, int G>
__global__ __launch_bounds__(DFB_THREADS) void k_dfb_factor(const double* __restrict__ A, int lda, long long stride, int upper, int n, int ld, int width, int batch,
                                                            double* __restrict__ F, int* __restrict__ info, int* __restrict__ badcol)
{
    extern __shared__ double dfb_lds[];
    constexpr int MPW = DFB_THREADS / G;
    __shared__ int s_fail[MPW];
    const int g = threadIdx.x / G, t = threadIdx.x % G;
    const long long mat = (long long)blockIdx.x * MPW + g;
    const bool have = mat < batch;
    double* a = dfb_lds + (size_t)g * n * ld;
    if (t == 0) s_fail[g] = -1;
    // element (i, j), i >= j, of the lower view; the walk is contiguous in the source for either triangle
    if (have) {
        const double* src = A + mat * stride;
        for (int e = t; e < n * n; e += G) {
            const int q = e / n, r = e % n;
            const int i = upper ? q : r, j = upper ? r : q;
            if (i >= j) a[i + j * ld] = src[r + (size_t)q * lda];
        }
    }
    __syncthreads();
    const bool live = dfb_factor_in_lds<KIND, G>(a, n, ld, width, have, g, t, s_fail);
    if (!have) return;
    if (t == 0) { info[mat] = live ? 0 : 1; badcol[mat] = s_fail[g]; }
    if (!live) return;
    double* dst = F + (size_t)mat * n * n;
    for (int e = t; e < n * n; e += G) {
        const int q = e / n, r = e % n;
        const int i = upper ? q : r, j = upper ? r : q;
        if (i >= j) dst[r + (size_t)q * n] = a[i + j * ld];
    }
}

// solveInPlace for DFB_NCH right-hand sides of one matrix: blockIdx.x = matrix, blockIdx.y = group of columns.  The factor comes from F (the handle's storage), the
// right-hand sides are staged in LDS as xs[row][column] so that the threads -- one per column -- sit on neighbouring banks.  A matrix whose factorisation failed
// returns at once: its block of X is not touched.
template <int KIND>
__global__ __launch_bounds__(DFB_SOLVE_THREADS) void k_dfb_solve(const double* __restrict__ F, const int* __restrict__ info, int n, int ld, int upper,
                                                                 double* __restrict__ X, int ldx, int nrhs, long long stride)
{
    extern __shared__ double dfb_lds[];
    const long long mat = blockIdx.x;
    if (info[mat] != 0) return;  // (uniform: before any barrier)
    double* a = dfb_lds;
    double* xs = dfb_lds + (size_t)n * ld;
    const int t = threadIdx.x;
    const double* src = F + (size_t)mat * n * n;
    for (int e = t; e < n * n; e += DFB_SOLVE_THREADS) {
        const int q = e / n, r = e % n;
        const int i = upper ? q : r, j = upper ? r : q;
        if (i >= j) a[i + j * ld] = src[r + (size_t)q * n];
    }
    const int c0 = blockIdx.y * DFB_NCH;
    const int nc = nrhs - c0 < DFB_NCH ? nrhs - c0 : DFB_NCH;
    double* xb = X + mat * stride + (size_t)c0 * ldx;
    for (int e = t; e < n * nc; e += DFB_SOLVE_THREADS) {
        const int c = e / n, i = e % n;
        xs[i * DFB_NCH + c] = xb[i + (size_t)c * ldx];
    }
    __syncthreads();
    if (t < nc) {
        double* x = xs + t;
        for (int j = 0; j < n; ++j) {
            double xj = x[j * DFB_NCH];
            if (KIND == 0) { xj = xj / a[j + j * ld]; x[j * DFB_NCH] = xj; }
            for (int i = j + 1; i < n; ++i) x[i * DFB_NCH] = fma(-a[i + j * ld], xj, x[i * DFB_NCH]);
        }
        if (KIND == 1)
            for (int j = 0; j < n; ++j) x[j * DFB_NCH] = x[j * DFB_NCH] / a[j + j * ld];
        for (int j = n - 1; j >= 0; --j) {
            const double* col = a + j * ld;
            const int count = n - 1 - j, even = count & ~1;
            double s = x[j * DFB_NCH];
            for (int q = 0; q < even; ++q) s = s - col[j + 1 + q] * x[(j + 1 + q) * DFB_NCH];
            if (count & 1) s = fma(-col[n - 1], x[(n - 1) * DFB_NCH], s);
            x[j * DFB_NCH] = KIND == 0 ? s / col[j] : s;
        }
    }
    __syncthreads();
    for (int e = t; e < n * nc; e += DFB_SOLVE_THREADS) {
        const int c = e / n, i = e % n;
        xb[i + (size_t)c * ldx] = xs[i * DFB_NCH + c];
    }
}

size_t factor_lds_bytes(int n) { return sizeof(double) * (size_t)n * dfb_ld(n) * (n < 32 ? DFB_THREADS / 64 : 1); }
size_t solve_lds_bytes(int n) { return sizeof(double) * ((size_t)n * dfb_ld(n) + (size_t)n * DFB_NCH); }

}  // namespace

}  // namespace pq

using namespace pq;

struct pq_dense_factor_batch {
    int device = 0, batch = 0, n = 0, kind = PQ_DENSE_LDLT_NO_PIVOT, uplo = PQ_LOWER, max_nrhs = 1;
    bool computed = false;
    DBuf<double> fac, stage_a, stage_x;
    DBuf<int> status;    // [0, batch): info, [batch, 2 batch): first bad column
    HBuf<int> status_h;
    HBuf<double> mat_h;  // n x n, pq_dense_factor_batch_matrix
    Event ev0, ev1;
    double last_ms[2] = {0.0, 0.0};
    Stream st;
};

extern "C" {

int pq_dense_factor_batch_create(pq_dense_factor_batch** out, int device, int batch, int n, int kind, int uplo, int max_nrhs)
{
    if (!out) return fail(PQ_ERR_INVALID, "null argument");
    if (batch < 1 || n < 1 || max_nrhs < 1) return fail(PQ_ERR_INVALID, "dense factor batch: batch, n and max_nrhs must be at least 1");
    if ((kind != PQ_DENSE_LDLT_NO_PIVOT && kind != PQ_DENSE_CHOLESKY) || (uplo != PQ_LOWER && uplo != PQ_UPPER)) return fail(PQ_ERR_INVALID, "dense factor batch: bad kind / uplo");
    if (n > PQ_DENSE_FACTOR_BATCH_MAX_N) return fail(PQ_ERR_UNSUPPORTED, "dense factor batch: n = %d, the limit is n <= %d", n, (int)PQ_DENSE_FACTOR_BATCH_MAX_N);
    return guarded([&] {
        PQ_HIP(hipSetDevice(device));
        std::unique_ptr<pq_dense_factor_batch> f(new pq_dense_factor_batch);
        f->device = device; f->batch = batch; f->n = n; f->kind = kind; f->uplo = uplo; f->max_nrhs = max_nrhs;
        f->st = Stream(device);
        const size_t nn = (size_t)n * n;
        f->fac.alloc(nn * batch); f->stage_a.alloc(nn * batch); f->stage_x.alloc((size_t)n * max_nrhs * batch);
        f->status.alloc(2 * (size_t)batch); f->status_h.alloc(2 * (size_t)batch); f->mat_h.alloc(nn);
        f->ev0 = Event(0);
        f->ev1 = Event(0);
        f->fac.zero(f->st);  // the triangle that is not named stays zero for life
        // the matrix at n = 128 (129 KiB, with sixteen right-hand sides 145 KiB) is more than the 64 KiB a launch may ask for by default
        static PerDeviceOnce once;
        once([&] {
            const int fb = (int)factor_lds_bytes(PQ_DENSE_FACTOR_BATCH_MAX_N), sb = (int)solve_lds_bytes(PQ_DENSE_FACTOR_BATCH_MAX_N);
            PQ_HIP(hipFuncSetAttribute((const void*)k_dfb_factor<0, DFB_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, fb));
            PQ_HIP(hipFuncSetAttribute((const void*)k_dfb_factor<1, DFB_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, fb));
            PQ_HIP(hipFuncSetAttribute((const void*)k_dfb_solve<0>, hipFuncAttributeMaxDynamicSharedMemorySize, sb));
            PQ_HIP(hipFuncSetAttribute((const void*)k_dfb_solve<1>, hipFuncAttributeMaxDynamicSharedMemorySize, sb));
        });
        stream_wait(f->st);
        *out = f.release();
        return (int)PQ_OK;
    });
}

void pq_dense_factor_batch_destroy(pq_dense_factor_batch* f) { delete f; }

int pq_dense_factor_batch_compute(pq_dense_factor_batch* f, const double* A, int lda, long long stride, int mem)
{
    if (!f || !A) return fail(PQ_ERR_INVALID, "null argument");
    if (lda < f->n || stride < (long long)lda * f->n) return fail(PQ_ERR_INVALID, "dense factor batch: lda < n or stride < lda * n");
    if (mem != PQ_MEM_HOST && mem != PQ_MEM_DEVICE) return fail(PQ_ERR_INVALID, "dense factor batch: bad mem");
    int good = 0;
    const int rc = guarded([&] {
        PQ_HIP(hipSetDevice(f->device));
        const int n = f->n, batch = f->batch;
        const auto w0 = std::chrono::steady_clock::now();
        hipStream_t st = f->st;
        const double* src = A;
        int ld = lda;
        long long str = stride;
        if (mem != PQ_MEM_DEVICE) {  // host matrices: packed into the staging buffer (leading dimension n, stride n n), the padding stays behind
            const size_t col = sizeof(double) * n;
            if (lda == n) PQ_HIP(hipMemcpy2DAsync(f->stage_a.p, col * n, A, sizeof(double) * stride, col * n, batch, hipMemcpyHostToDevice, st));
            else
                for (int b = 0; b < batch; ++b)
                    PQ_HIP(hipMemcpy2DAsync(f->stage_a.p + (size_t)b * n * n, col, A + (size_t)b * stride, sizeof(double) * lda, col, n, hipMemcpyHostToDevice, st));
            src = f->stage_a.p; ld = n; str = (long long)n * n;
        }
        const int upper = f->uplo == PQ_UPPER, ldl = dfb_ld(n);
        const size_t lds = factor_lds_bytes(n);
        PQ_HIP(hipEventRecord(f->ev0, st));
        if (n < 32) {
            const int grid = div_up(batch, DFB_THREADS / 64);
            if (f->kind == PQ_DENSE_CHOLESKY) k_dfb_factor<0, 64><<<grid, DFB_THREADS, lds, st>>>(src, ld, str, upper, n, ldl, n, batch, f->fac.p, f->status.p, f->status.p + batch);
            else k_dfb_factor<1, 64><<<grid, DFB_THREADS, lds, st>>>(src, ld, str, upper, n, ldl, n, batch, f->fac.p, f->status.p, f->status.p + batch);
        } else {
            const int width = dfb_block_size_rule(n);
            if (f->kind == PQ_DENSE_CHOLESKY) k_dfb_factor<0, DFB_THREADS><<<batch, DFB_THREADS, lds, st>>>(src, ld, str, upper, n, ldl, width, batch, f->fac.p, f->status.p, f->status.p + batch);
            else k_dfb_factor<1, DFB_THREADS><<<batch, DFB_THREADS, lds, st>>>(src, ld, str, upper, n, ldl, width, batch, f->fac.p, f->status.p, f->status.p + batch);
        }
        PQ_HIP(hipGetLastError());
        PQ_HIP(hipEventRecord(f->ev1, st));
        PQ_HIP(hipMemcpyAsync(f->status_h.p, f->status.p, sizeof(int) * 2 * batch, hipMemcpyDeviceToHost, st));
        stream_wait(st);
        float ms = 0.f;
        PQ_HIP(hipEventElapsedTime(&ms, f->ev0, f->ev1));
        f->last_ms[0] = ms;
        f->last_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        for (int b = 0; b < batch; ++b) good += f->status_h.p[b] == 0;
        f->computed = true;
        return (int)PQ_OK;
    });
    return rc == PQ_OK ? good : rc;
}

int pq_dense_factor_batch_info(const pq_dense_factor_batch* f, int* info_host, int* first_bad_col_host)
{
    if (!f || !info_host) return fail(PQ_ERR_INVALID, "null argument");
    if (!f->computed) return fail(PQ_ERR_INVALID, "dense factor batch: no factorisation yet");
    for (int b = 0; b < f->batch; ++b) {
        info_host[b] = f->status_h.p[b];
        if (first_bad_col_host) first_bad_col_host[b] = f->status_h.p[f->batch + b];
    }
    return PQ_OK;
}

int pq_dense_factor_batch_solve_in_place(pq_dense_factor_batch* f, double* X, int ldx, int nrhs, long long stride, int mem)
{
    if (!f || !X) return fail(PQ_ERR_INVALID, "null argument");
    if (!f->computed) return fail(PQ_ERR_INVALID, "dense factor batch: solve before compute");
    if (nrhs < 1 || nrhs > f->max_nrhs) return fail(PQ_ERR_INVALID, "dense factor batch: nrhs = %d outside [1, max_nrhs = %d]", nrhs, f->max_nrhs);
    if (ldx < f->n || stride < (long long)ldx * nrhs) return fail(PQ_ERR_INVALID, "dense factor batch: ldx < n or stride < ldx * nrhs");
    if (mem != PQ_MEM_HOST && mem != PQ_MEM_DEVICE) return fail(PQ_ERR_INVALID, "dense factor batch: bad mem");
    return guarded([&] {
        PQ_HIP(hipSetDevice(f->device));
        const int n = f->n, batch = f->batch;
        hipStream_t st = f->st;
        double* xd = X;
        int ld = ldx;
        long long str = stride;
        const size_t col = sizeof(double) * n;
        const bool host = mem != PQ_MEM_DEVICE;
        if (host) {
            if (ldx == n) PQ_HIP(hipMemcpy2DAsync(f->stage_x.p, col * nrhs, X, sizeof(double) * stride, col * nrhs, batch, hipMemcpyHostToDevice, st));
            else
                for (int b = 0; b < batch; ++b)
                    PQ_HIP(hipMemcpy2DAsync(f->stage_x.p + (size_t)b * n * nrhs, col, X + (size_t)b * stride, sizeof(double) * ldx, col, nrhs, hipMemcpyHostToDevice, st));
            xd = f->stage_x.p; ld = n; str = (long long)n * nrhs;
        }
        const dim3 grid(batch, div_up(nrhs, DFB_NCH));
        const int upper = f->uplo == PQ_UPPER;
        if (f->kind == PQ_DENSE_CHOLESKY) k_dfb_solve<0><<<grid, DFB_SOLVE_THREADS, solve_lds_bytes(n), st>>>(f->fac.p, f->status.p, n, dfb_ld(n), upper, xd, ld, nrhs, str);
        else k_dfb_solve<1><<<grid, DFB_SOLVE_THREADS, solve_lds_bytes(n), st>>>(f->fac.p, f->status.p, n, dfb_ld(n), upper, xd, ld, nrhs, str);
        PQ_HIP(hipGetLastError());
        if (host) {  // (the block of a failed matrix comes back as it went: the kernel left the staged copy alone)
            if (ldx == n) PQ_HIP(hipMemcpy2DAsync(X, sizeof(double) * stride, f->stage_x.p, col * nrhs, col * nrhs, batch, hipMemcpyDeviceToHost, st));
            else
                for (int b = 0; b < batch; ++b)
                    PQ_HIP(hipMemcpy2DAsync(X + (size_t)b * stride, sizeof(double) * ldx, f->stage_x.p + (size_t)b * n * nrhs, col, col, nrhs, hipMemcpyDeviceToHost, st));
        }
        stream_wait(st);
        return (int)PQ_OK;
    });
}

int pq_dense_factor_batch_matrix(pq_dense_factor_batch* f, int instance, double* out_host, int ldo)
{
    if (!f || !out_host) return fail(PQ_ERR_INVALID, "null argument");
    if (!f->computed) return fail(PQ_ERR_INVALID, "dense factor batch: no factorisation yet");
    if (instance < 0 || instance >= f->batch) return fail(PQ_ERR_INVALID, "dense factor batch: instance %d outside [0, %d)", instance, f->batch);
    if (ldo < f->n) return fail(PQ_ERR_INVALID, "dense factor batch: ldo < n");
    return guarded([&] {
        PQ_HIP(hipSetDevice(f->device));
        const int n = f->n;
        PQ_HIP(hipMemcpyAsync(f->mat_h.p, f->fac.p + (size_t)instance * n * n, sizeof(double) * n * n, hipMemcpyDeviceToHost, f->st));
        stream_wait(f->st);
        for (int j = 0; j < n; ++j)
            for (int i = j; i < n; ++i) {
                if (f->uplo == PQ_LOWER) out_host[i + (size_t)j * ldo] = f->mat_h.p[i + (size_t)j * n];
                else out_host[j + (size_t)i * ldo] = f->mat_h.p[j + (size_t)i * n];
            }
        return (int)PQ_OK;
    });
}

int pq_dense_factor_batch_last_ms(const pq_dense_factor_batch* f, double out2[2])
{
    if (!f || !out2) return fail(PQ_ERR_INVALID, "null argument");
    out2[0] = f->last_ms[0]; out2[1] = f->last_ms[1];
    return PQ_OK;
}

}  // extern "C"
