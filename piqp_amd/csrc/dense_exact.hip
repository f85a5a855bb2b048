// piqp_amd/csrc/dense_exact.hip -- the dense KKT backend in the REFERENCE'S OWN ORDER of floating-point operations (kkt_solver = PQ_DENSE_CHOLESKY_EXACT, n <= 1024).
//
// Every member performs, per output element, the sequence of IEEE operations the CPU oracle's dense backend performs (oracle/orc_dense.c as oracle/Makefile builds it:
// -ffp-contract=fast, so its multiply-adds are fused), hence the assembled matrix, the factor, every solve and every mat-vec are the oracle's bit for bit.  This file
// is compiled with -ffp-contract=off (piqp_amd/build.py, NO_CONTRACT): every fused operation below is an explicit fma(), everything else rounds on its own.  Each
// element is one sequential chain and elements are independent, so the parallelism is across elements; no matrix instruction is used (its internal summation is not
// the oracle's).
//
//   oracle (orc_dense.c)                      here
//   syrk_like_lower                           k_ex_syrk: per K block of 256, acc = 0, acc = fma(a[i][k], w[k] * a[j][k], acc) for ascending k, then C += acc
//   dense_update_kkt                          the prologue of k_ex_syrk: P_utri^T, + x_reg on the diagonal, fma(1 / delta, AT_A, .)
//   orc_llt_compute / llt_unblocked /         k_ex_panel, one launch per panel of block_size_rule(n) columns (one launch in all below n = 32).  The reference is
//   trsm_right_lower_trans                    right-looking: panel k subtracts its product from everything to its right.  An element therefore receives one
//                                             subtraction per earlier panel, panel 0's first; the launch of panel k applies exactly these, in this order, to the
//                                             elements of ITS columns before it factors them (left-looking, the same operations per element).  Every workgroup
//                                             updates and factors the diagonal block for itself in LDS (same bits everywhere: no hand-over between workgroups
//                                             inside a launch), then solves its own 64 rows of the panel.  A launch reads the assembled matrix and the finished
//                                             columns of the factor and writes only its own panel's columns, so its workgroups need no order (see k_ex_panel)
//   orc_llt_solve_inplace                     k_ex_sweeps: column-oriented forward sweep (one thread per row), dot-product backward sweep (one chain per output)
//   gemv_n / gemv_t / dense_eval_P_x          k_ex_rhs, k_ex_gemv_n, k_ex_gemv_t, k_ex_eval_P: one thread per output element, ascending index
#include <cmath>
#include <stdexcept>

#include "kkt_solver_base.hpp"

namespace pq {

namespace {

constexpr int EX_MAX_N = 1024;  // one thread per row in the sweeps, one workgroup
constexpr int EX_KC = 256;      // K block of syrk_like_lower
constexpr int EX_RB = 64;       // rows of a panel per workgroup

// dense/ldlt_no_pivot.hpp:321-323 == Eigen LLT.h blocked()
int block_size_rule(int size)
{
    int bs = size / 8;
    bs = (bs / 16) * 16;
    if (bs < 8) bs = 8;
    if (bs > 128) bs = 128;
    return bs;
}

// ---- assembly and AT_A: C_lower = init + sum over K blocks of (chain from zero).  32 x 32 tile per workgroup of 256, 2 x 2 elements per thread, operands staged
// through LDS 16 columns of K at a time (16 divides 256, so a K block boundary is a stage boundary).  Pu != nullptr: init = P_utri^T (+ x_reg on the diagonal,
// then fma(dinv, AT_A, .) when ATA != nullptr); Pu == nullptr: init = 0 (the memset of dense_compute_ATA; 0 + acc, not acc: they differ for acc = -0).
__global__ __launch_bounds__(256) void k_ex_syrk(int n, int kdim, const double* __restrict__ A, int lda, const double* __restrict__ w, const double* __restrict__ Pu,
                                                 const double* __restrict__ x_reg, const double* __restrict__ ATA, double dinv, double* __restrict__ C, int ldc)
{
    const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    if (j0 > i0 + 31) return;  // (a tile entirely above the diagonal)
    __shared__ double As[16][33], Bs[16][33];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double c[2][2], acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const int i = i0 + tx + 16 * a, j = j0 + ty + 16 * b;
            double v = 0.0;
            if (Pu && i < n && j < n && i >= j) {
                v = Pu[j + (size_t)i * n];
                if (i == j) v = v + x_reg[j];
                if (ATA) v = fma(dinv, ATA[i + (size_t)j * n], v);
            }
            c[a][b] = v;
            acc[a][b] = 0.0;
        }
    const int sr = threadIdx.x & 31, sk = threadIdx.x >> 5;
    for (int k0 = 0; k0 < kdim; k0 += 16) {
        if (k0 > 0 && k0 % EX_KC == 0)
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) { c[a][b] = c[a][b] + acc[a][b]; acc[a][b] = 0.0; }
        __syncthreads();
        for (int h = 0; h < 2; ++h) {
            const int kk = sk + 8 * h, k = k0 + kk;
            double va = 0.0, vb = 0.0;
            if (k < kdim) {
                if (i0 + sr < n) va = A[(i0 + sr) + (size_t)k * lda];
                if (j0 + sr < n) { vb = A[(j0 + sr) + (size_t)k * lda]; if (w) vb = w[k] * vb; vb = 0.0 + vb; }  // (the micro-kernel's broadcast is (vd){0} + b: -0 becomes +0)
            }
            As[kk][sr] = va;
            Bs[kk][sr] = vb;
        }
        __syncthreads();
        const int kmax = kdim - k0 < 16 ? kdim - k0 : 16;
        for (int kk = 0; kk < kmax; ++kk) {
            const double a0 = As[kk][tx], a1 = As[kk][tx + 16], b0 = Bs[kk][ty], b1 = Bs[kk][ty + 16];
            acc[0][0] = fma(a0, b0, acc[0][0]);
            acc[0][1] = fma(a0, b1, acc[0][1]);
            acc[1][0] = fma(a1, b0, acc[1][0]);
            acc[1][1] = fma(a1, b1, acc[1][1]);
        }
    }
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const int i = i0 + tx + 16 * a, j = j0 + ty + 16 * b;
            if (i < n && j < n && i >= j) C[i + (size_t)j * ldc] = kdim > 0 ? c[a][b] + acc[a][b] : c[a][b];
        }
}

// ---- factorisation
__device__ __forceinline__ int tri(int bs, int i, int j) { return j * bs - (j * (j - 1)) / 2 + (i - j); }  // packed lower triangle by columns

// Elements (row, col0 .. col0 + 3) of the panel that starts at column k, brought up to date: one subtraction per earlier panel (columns c0 .. c0 + width), each the
// chain from zero over that panel's columns (syrk_like_lower with alpha = -1, K = width <= 128: one K block).  ncol <= 4 valid columns.  The starting values come
// from src, the assembled matrix, which no launch of the factorisation writes; `a`, the factor, is read at columns < k only (finished by earlier launches).
__device__ __forceinline__ void ex_update4(const double* __restrict__ src, const double* a, int lda, int row, int col0, int ncol, int k, int width, double c[4])
{
    int cq[4];
    for (int q = 0; q < 4; ++q) {
        cq[q] = col0 + (q < ncol ? q : 0);
        c[q] = src[row + (size_t)cq[q] * lda];
    }
    for (int c0 = 0; c0 < k; c0 += width) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int kk = 0; kk < width; ++kk) {
            const size_t off = (size_t)(c0 + kk) * lda;
            const double li = a[row + off];
            for (int q = 0; q < 4; ++q) acc[q] = fma(li, 0.0 + a[cq[q] + off], acc[q]);  // (0 + b: the micro-kernel's broadcast)
        }
        for (int q = 0; q < 4; ++q) c[q] = c[q] - acc[q];
    }
}

// One panel: columns k .. k + bs of the factor a of the n x n matrix src (lower triangles, column-major, same leading dimension).  Grid: max(1, ceil((n - k - bs) / 64))
// workgroups of 256.  Race-free without any ordering between the workgroups of a launch: a launch READS src (written by the assembly only) and the columns < k of a
// (written by earlier launches on the same stream), and WRITES the columns k .. k + bs of a -- the diagonal block by workgroup 0, rows row0 .. row0 + 64 by their owner --
// which no workgroup of this launch reads.  (Starting from a copy of src inside a would let a late workgroup read workgroup 0's finished L11 for A11.)
// Dynamic LDS: bs (bs + 1) / 2 doubles (the diagonal block, packed) + 64 bs doubles (this workgroup's rows of the panel, column by column).
// info[0]: -1, or the column of the first pivot with !(x > 0) (Eigen LLT: NumericalIssue); a launch that finds it set does nothing.
__global__ __launch_bounds__(256) void k_ex_panel(const double* __restrict__ src, double* a, int n, int lda, int k, int bs, int width, int* __restrict__ info)
{
    extern __shared__ double ex_lds[];
    __shared__ int fail;
    if (*(volatile int*)info != -1) return;
    double* Ld = ex_lds;
    double* Xr = ex_lds + (bs * (bs + 1)) / 2;
    const int tid = threadIdx.x, r = tid & 63, jg = tid >> 6;
    const int row0 = k + bs + (int)blockIdx.x * EX_RB;
    if (tid == 0) fail = -1;
    // the diagonal block, up to date, into LDS
    for (int rc = 0; rc < bs; rc += 64) {
        const int i = rc + r;
        if (i >= bs) continue;
        for (int jq = jg * 4; jq <= i; jq += 16) {
            const int ncol = (i - jq + 1) < 4 ? (i - jq + 1) : 4;
            double c[4];
            ex_update4(src, a, lda, k + i, k + jq, ncol, k, width, c);
            for (int q = 0; q < ncol; ++q) Ld[tri(bs, i, jq + q)] = c[q];
        }
    }
    // this workgroup's rows of the panel, up to date, into LDS
    const bool has_row = row0 + r < n;
    if (has_row)
        for (int jq = jg * 4; jq < bs; jq += 16) {
            const int ncol = (bs - jq) < 4 ? (bs - jq) : 4;
            double c[4];
            ex_update4(src, a, lda, row0 + r, k + jq, ncol, k, width, c);
            for (int q = 0; q < ncol; ++q) Xr[(jq + q) * EX_RB + r] = c[q];
        }
    __syncthreads();
    // llt_unblocked on the diagonal block: thread i owns row i
    for (int kc = 0; kc < bs; ++kc) {
        double c = 0.0;
        if (tid == kc) {
            double x = Ld[tri(bs, kc, kc)];
            if (kc > 0) {
                double s = 0.0;
                for (int j = 0; j < kc; ++j) { const double v = Ld[tri(bs, kc, j)]; s = fma(v, v, s); }
                x = x - s;
            }
            if (!(x > 0.0)) fail = kc;
            else Ld[tri(bs, kc, kc)] = sqrt(x);
        } else if (tid > kc && tid < bs) {
            c = Ld[tri(bs, tid, kc)];
            for (int j = 0; j < kc; ++j) c = fma(-Ld[tri(bs, tid, j)], Ld[tri(bs, kc, j)], c);
        }
        __syncthreads();
        if (fail >= 0) break;
        if (tid > kc && tid < bs) Ld[tri(bs, tid, kc)] = c / Ld[tri(bs, kc, kc)];
        __syncthreads();
    }
    if (fail >= 0) {
        if (blockIdx.x == 0 && tid == 0) info[0] = k + fail;
        return;
    }
    if (blockIdx.x == 0)
        for (int j = 0; j < bs; ++j)
            for (int i = j + tid; i < bs; i += 256) a[(k + i) + (size_t)(k + j) * lda] = Ld[tri(bs, i, j)];
    // trsm_right_lower_trans: row by row, x_j = (a_j - sum_{kk < j} x_kk l_jkk) / l_jj with the sum taken as fma(-x_kk, l_jkk, .) for ascending kk
    if (tid < EX_RB && has_row)
        for (int j = 0; j < bs; ++j) {
            double c = Xr[j * EX_RB + r];
            for (int kk = 0; kk < j; ++kk) c = fma(-Xr[kk * EX_RB + r], Ld[tri(bs, j, kk)], c);
            Xr[j * EX_RB + r] = c / Ld[tri(bs, j, j)];
        }
    __syncthreads();
    if (has_row)
        for (int j = jg; j < bs; j += 4) a[(row0 + r) + (size_t)(k + j) * lda] = Xr[j * EX_RB + r];
}

// ---- solve
// The oracle's dot products over contiguous memory (gemv_t, the backward sweep, dense_eval_P_x) are vectorised by its compiler as in-order reductions: the products
// of the vector body are rounded on their own and added in ascending order, and only the scalar tail -- the last element of an odd count -- is a fused
// multiply-add (objdump of oracle/_build/orc_dense.o: vmulpd + vaddsd x 4, vmulpd + vaddsd x 2, vfmadd231sd).  Strided chains (llt_unblocked's) are fused throughout.
__device__ __forceinline__ double ex_dot(const double* __restrict__ a, const double* __restrict__ b, int count)
{
    double s = 0.0;
    const int even = count & ~1;
    for (int i = 0; i < even; ++i) s = s + a[i] * b[i];
    if (count & 1) s = fma(a[count - 1], b[count - 1], s);
    return s;
}

__global__ void k_ex_reciprocal(int m, const double* __restrict__ z, double* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = 1.0 / z[i];
}

// dense_solve, the right-hand side: lhs_x = rhs_x, then gemv_n with GT and work_z = z_reg_inv o rhs_z, then gemv_n with AT and delta_inv * rhs_y
__global__ void k_ex_rhs(int n, int p, int m, const double* __restrict__ GT, const double* __restrict__ AT, const double* __restrict__ zinv, double delta_inv,
                         const double* __restrict__ rhs_x, const double* __restrict__ rhs_y, const double* __restrict__ rhs_z, double* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double c = rhs_x[i];
    for (int j = 0; j < m; ++j) c = fma(GT[i + (size_t)j * n], zinv[j] * rhs_z[j], c);
    for (int j = 0; j < p; ++j) c = fma(AT[i + (size_t)j * n], delta_inv * rhs_y[j], c);
    out[i] = c;
}

// orc_llt_solve_inplace: one workgroup of 1024, thread i owns x[i].  Forward: for ascending j, x_j = x_j / l_jj, then x_i = fma(-l_ij, x_j, x_i) for every i > j.
// Backward: for descending j, s = x_j, s = s - l_ij x_i for ascending i > j (ex_dot's rule: products rounded on their own, the last of an odd count fused),
// x_j = s / l_jj -- a chain that starts at the value finished last, so the whole sweep is one dependent chain of n^2 / 2 subtractions (thread 0 walks it; the
// others multiply and stage the next column in LDS meanwhile).
__global__ __launch_bounds__(1024) void k_ex_sweeps(const double* __restrict__ L, int n, int lda, double* __restrict__ x)
{
    __shared__ double xs[EX_MAX_N], Ls[2][EX_MAX_N], pr[2][EX_MAX_N], xb[2];
    const int i = threadIdx.x;
    const bool in = i < n;
    double c = in ? x[i] : 0.0;
    double lnext = in ? L[i] : 1.0;
    for (int j = 0; j < n; ++j) {
        const double l = lnext;
        if (in && j + 1 < n) lnext = L[i + (size_t)(j + 1) * lda];
        if (i == j) { c = c / l; xb[j & 1] = c; }
        __syncthreads();
        if (in && i > j) c = fma(-l, xb[j & 1], c);
    }
    xs[i] = c;
    __syncthreads();
    lnext = in ? L[i + (size_t)(n - 1) * lda] : 1.0;
    for (int j = n - 1; j >= 0; --j) {
        // column j and its products with the values that are final by now (x[j + 1] is not: thread 0 multiplies that one itself)
        Ls[j & 1][i] = lnext;
        if (in && i >= j + 2) pr[j & 1][i] = lnext * xs[i];
        if (in && j > 0) lnext = L[i + (size_t)(j - 1) * lda];
        __syncthreads();
        if (i == 0) {
            const double* col = Ls[j & 1];
            const double* prod = pr[j & 1];
            const int count = n - 1 - j, even = count & ~1;
            double s = xs[j];
            if (even > 0) s = s - col[j + 1] * xs[j + 1];
#pragma unroll 8
            for (int q = 1; q < even; ++q) s = s - prod[j + 1 + q];
            if (count & 1) s = fma(-col[n - 1], xs[n - 1], s);
            xs[j] = s / col[j];
        }
    }
    __syncthreads();
    if (in) x[i] = xs[i];
}

// gemv_t: y[j] = alpha * ex_dot(column j of A, x), one thread per output, with dense_solve's two epilogues:
//   mode 1  lhs_y[j] = fma(-alpha, sub[j], y[j])         (lhs_y[i] -= delta_inv * rhs_y[i], contracted)
//   mode 2  lhs_z[j] = (y[j] - sub[j]) * scale[j]
__global__ void k_ex_gemv_t(int rows, int cols, const double* __restrict__ A, int lda, const double* __restrict__ x, double alpha, int mode,
                            const double* __restrict__ sub, const double* __restrict__ scale, double* __restrict__ y)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    const double* col = A + (size_t)j * lda;
    const double s = ex_dot(col, x, rows);
    double v = alpha * s;
    if (mode == 1) v = fma(-alpha, sub[j], v);
    if (mode == 2) { v = v - sub[j]; v = v * scale[j]; }
    y[j] = v;
}

// gemv_n into a zeroed vector: y[i] = chain over ascending j of fma(A[i][j], alpha * x[j], .)
__global__ void k_ex_gemv_n(int rows, int cols, const double* __restrict__ A, int lda, const double* __restrict__ x, double alpha, double* __restrict__ y)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    double c = 0.0;
    for (int j = 0; j < cols; ++j) c = fma(A[i + (size_t)j * lda], alpha * x[j], c);
    y[i] = c;
}

// dense_eval_P_x.  z[t] is touched first by column t (z[t] is still zero then): z[t] = 0 + fma(P_tt, alpha x_t, alpha * s_t) with s_t = ex_dot over the part of
// column t above the diagonal; after that by every column j > t: z[t] = fma(P_tj, alpha x_j, z[t]).
__global__ void k_ex_eval_P(int n, const double* __restrict__ Pu, double alpha, const double* __restrict__ x, double* __restrict__ z)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double* col = Pu + (size_t)t * n;
    const double s = ex_dot(col, x, t);
    double v = 0.0 + fma(col[t], alpha * x[t], alpha * s);
    for (int j = t + 1; j < n; ++j) v = fma(Pu[t + (size_t)j * n], alpha * x[j], v);
    z[t] = v;
}

__global__ void k_ex_diag(int n, const double* __restrict__ Pu, double* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = Pu[i + (size_t)i * n];
}

// test hook (pq_debug_device_sqrt): out[i] = sqrt(in[i]) as the factorisation kernel computes it
__global__ void k_ex_sqrt(long long count, const double* __restrict__ in, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = sqrt(in[i]);
}

inline void check_launch() { PQ_HIP(hipGetLastError()); }

class DenseExactKKT final : public KKTSolverBase {
public:
    DenseExactKKT(const pq_dense_data* d, int device) : dev_(device), n_(d->n), p_(d->p), m_(d->m)
    {
        if (n_ <= 0 || p_ < 0 || m_ < 0) throw std::runtime_error("dense KKT: bad dimensions");
        if (n_ > EX_MAX_N) throw std::runtime_error("dense_cholesky_exact: n <= 1024 only");
        st_ = Stream(dev_);
        alloc();
        upload(d);
    }

    std::unique_ptr<KKTSolverBase> clone() const override
    {
        PQ_HIP(hipSetDevice(dev_));
        stream_wait(st_);
        return std::unique_ptr<KKTSolverBase>(new DenseExactKKT(*this, 0));  // (a private constructor)
    }

    // dense/kkt.hpp:62-71 (every call refreshes all three matrices and AT_A, like the other dense backend: Solver::update rewrites them even when none is passed)
    void update_data_dense(const pq_dense_data* d, int options) override
    {
        (void)options;
        if (d->n != n_ || d->p != p_ || d->m != m_) throw std::runtime_error("update_data: dimension mismatch");
        PQ_HIP(hipSetDevice(dev_));
        upload(d);
    }

    // dense/kkt.hpp:73-84
    bool update_scalings_and_factor(double delta, const double* x_reg, const double* z_reg) override
    {
        PQ_HIP(hipSetDevice(dev_));
        delta_ = delta;
        const double dinv = 1.0 / delta_;
        const int nt = div_up(n_, 32);
        const int t0 = prof_.begin(0, st_);
        if (m_ > 0) { k_ex_reciprocal<<<div_up(m_, 256), 256, 0, st_>>>(m_, z_reg, z_reg_inv_.p); check_launch(); }
        k_ex_syrk<<<dim3(nt, nt), 256, 0, st_>>>(n_, m_, GT_.p, n_, z_reg_inv_.p, Pu_.p, x_reg, p_ > 0 ? ATA_.p : nullptr, dinv, kkt_.p, n_);
        check_launch();
        prof_.end(0, t0, st_);
        const int t1 = prof_.begin(1, st_);
        // llt.compute(kkt_mat) factors a copy: here every panel launch takes its starting values from kkt_ and writes its columns of the factor into fac_
        PQ_HIP(hipMemsetAsync(info_.p, 0xFF, sizeof(int), st_));  // -1
        const int width = n_ < 32 ? n_ : block_size_rule(n_);
        for (int k = 0; k < n_; k += width) {
            const int bs = n_ - k < width ? n_ - k : width;
            const int rs = n_ - k - bs;
            const int grid = rs > 0 ? div_up(rs, EX_RB) : 1;
            k_ex_panel<<<grid, 256, panel_lds_bytes(bs), st_>>>(kkt_.p, fac_.p, n_, n_, k, bs, width, info_.p);
            check_launch();
        }
        prof_.end(1, t1, st_);
        PQ_HIP(hipMemcpyAsync(info_h_.p, info_.p, sizeof(int), hipMemcpyDeviceToHost, st_));
        stream_wait(st_);
        return info_h_.p[0] == -1;
    }

    // dense/kkt.hpp:86-105
    void solve(const double* rhs_x, const double* rhs_y, const double* rhs_z, double* lhs_x, double* lhs_y, double* lhs_z) override
    {
        PQ_HIP(hipSetDevice(dev_));
        const double delta_inv = 1.0 / delta_;
        const int tk = prof_.begin(2, st_);
        k_ex_rhs<<<div_up(n_, 64), 64, 0, st_>>>(n_, p_, m_, GT_.p, AT_.p, z_reg_inv_.p, delta_inv, rhs_x, rhs_y, rhs_z, lhs_x);
        check_launch();
        k_ex_sweeps<<<1, 1024, 0, st_>>>(fac_.p, n_, n_, lhs_x);
        check_launch();
        if (p_ > 0) { k_ex_gemv_t<<<div_up(p_, 64), 64, 0, st_>>>(n_, p_, AT_.p, n_, lhs_x, delta_inv, 1, rhs_y, nullptr, lhs_y); check_launch(); }
        if (m_ > 0) { k_ex_gemv_t<<<div_up(m_, 64), 64, 0, st_>>>(n_, m_, GT_.p, n_, lhs_x, 1.0, 2, rhs_z, z_reg_inv_.p, lhs_z); check_launch(); }
        prof_.end(2, tk, st_);
    }

    // dense/kkt.hpp:108-114
    void eval_P_x(double alpha, const double* x, double* z) override
    {
        PQ_HIP(hipSetDevice(dev_));
        k_ex_eval_P<<<div_up(n_, 64), 64, 0, st_>>>(n_, Pu_.p, alpha, x, z);
        check_launch();
    }
    // dense/kkt.hpp:117-123
    void eval_A_xn_and_AT_xt(double alpha_n, double alpha_t, const double* xn, const double* xt, double* zn, double* zt) override
    {
        PQ_HIP(hipSetDevice(dev_));
        if (p_ > 0) { k_ex_gemv_t<<<div_up(p_, 64), 64, 0, st_>>>(n_, p_, AT_.p, n_, xn, alpha_n, 0, nullptr, nullptr, zn); check_launch(); }
        k_ex_gemv_n<<<div_up(n_, 64), 64, 0, st_>>>(n_, p_, AT_.p, n_, xt, alpha_t, zt);
        check_launch();
    }
    // dense/kkt.hpp:126-132
    void eval_G_xn_and_GT_xt(double alpha_n, double alpha_t, const double* xn, const double* xt, double* zn, double* zt) override
    {
        PQ_HIP(hipSetDevice(dev_));
        if (m_ > 0) { k_ex_gemv_t<<<div_up(m_, 64), 64, 0, st_>>>(n_, m_, GT_.p, n_, xn, alpha_n, 0, nullptr, nullptr, zn); check_launch(); }
        k_ex_gemv_n<<<div_up(n_, 64), 64, 0, st_>>>(n_, m_, GT_.p, n_, xt, alpha_t, zt);
        check_launch();
    }

    const double* P_diag_device() const override { return Pdiag_.p; }
    int n() const override { return n_; }
    int p() const override { return p_; }
    int m() const override { return m_; }
    hipStream_t stream() const override { return st_; }
    int device() const override { return dev_; }
    bool reference_order() const override { return true; }

    // hipEvent brackets as in the other dense backend: stage 0 assembly, 1 factorisation, 2 solve
    void set_profiling(int level) override { prof_.enabled = level != 0; prof_.level = level; }
    void get_profile(int stage, double* total_ms, int* count) override
    {
        if (stage < 0 || stage >= StageProfiler::NSTAGE) throw std::runtime_error("bad stage");
        PQ_HIP(hipSetDevice(dev_));
        prof_.collect(stage, st_, total_ms, count);
    }
    void internal_kkt_mat(double* out_host) override { download(kkt_, out_host); }
    void internal_factor(double* out_host) override { download(fac_, out_host); }

private:
    DenseExactKKT(const DenseExactKKT& o, int) : dev_(o.dev_), n_(o.n_), p_(o.p_), m_(o.m_), delta_(o.delta_)
    {
        st_ = Stream(dev_);
        alloc();
        copy_state(o);
    }

    void copy_state(const DenseExactKKT& o)
    {
        auto cp = [&](DBuf<double>& dst, const DBuf<double>& src) { if (src.n) PQ_HIP(hipMemcpyAsync(dst.p, src.p, src.bytes(), hipMemcpyDeviceToDevice, st_)); };
        cp(Pu_, o.Pu_); cp(Pdiag_, o.Pdiag_); cp(AT_, o.AT_); cp(GT_, o.GT_); cp(ATA_, o.ATA_); cp(kkt_, o.kkt_); cp(fac_, o.fac_); cp(z_reg_inv_, o.z_reg_inv_);
        stream_wait(st_);
    }

    static size_t panel_lds_bytes(int bs) { return sizeof(double) * ((size_t)(bs * (bs + 1)) / 2 + (size_t)EX_RB * bs); }

    void alloc()
    {
        const size_t nn = (size_t)n_ * n_;
        Pu_.alloc(nn); Pdiag_.alloc(n_);
        AT_.alloc((size_t)n_ * p_); GT_.alloc((size_t)n_ * m_);
        if (p_ > 0) ATA_.alloc(nn);
        kkt_.alloc(nn); fac_.alloc(nn);
        z_reg_inv_.alloc(m_);
        info_.alloc(1); info_h_.alloc(1);
        info_h_.p[0] = -1;
        kkt_.zero(st_); fac_.zero(st_);
        // the widest panel's diagonal block and row block: 66 + 64 KiB of the compute unit's 160 KiB of LDS
        static PerDeviceOnce once;
        once([&] { PQ_HIP(hipFuncSetAttribute((const void*)k_ex_panel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)panel_lds_bytes(128))); });
    }

    void upload(const pq_dense_data* d)
    {
        copy_in(Pu_.p, d->P_utri, (size_t)n_ * n_ * sizeof(double), d->mem, st_);
        copy_in(AT_.p, d->AT, (size_t)n_ * p_ * sizeof(double), d->mem, st_);
        copy_in(GT_.p, d->GT, (size_t)n_ * m_ * sizeof(double), d->mem, st_);
        k_ex_diag<<<div_up(n_, 256), 256, 0, st_>>>(n_, Pu_.p, Pdiag_.p);
        check_launch();
        if (p_ > 0) {
            // dense/kkt.hpp:53 AT_A.lower = AT * AT^T
            const int nt = div_up(n_, 32);
            k_ex_syrk<<<dim3(nt, nt), 256, 0, st_>>>(n_, p_, AT_.p, n_, nullptr, nullptr, nullptr, nullptr, 0.0, ATA_.p, n_);
            check_launch();
        }
        stream_wait(st_);  // host source buffers may be released by the caller after return
    }

    void download(const DBuf<double>& src, double* out_host)
    {
        PQ_HIP(hipSetDevice(dev_));
        PQ_HIP(hipMemcpyAsync(out_host, src.p, src.bytes(), hipMemcpyDeviceToHost, st_));
        stream_wait(st_);
    }

    int dev_, n_, p_, m_;
    double delta_ = 1.0;
    DBuf<double> Pu_, Pdiag_, AT_, GT_, ATA_, kkt_, fac_, z_reg_inv_;
    DBuf<int> info_;
    HBuf<int> info_h_;
    StageProfiler prof_;
    Stream st_;
};

}  // namespace

std::unique_ptr<KKTSolverBase> make_dense_exact_kkt(const pq_dense_data* data, int device) { return std::make_unique<DenseExactKKT>(data, device); }

void debug_device_sqrt(const double* in_host, double* out_host, long long count, int device)
{
    PQ_HIP(hipSetDevice(device));
    DBuf<double> in((size_t)count), out((size_t)count);
    PQ_HIP(hipMemcpy(in.p, in_host, in.bytes(), hipMemcpyHostToDevice));
    k_ex_sqrt<<<(unsigned)((count + 255) / 256), 256>>>(count, in.p, out.p);
    check_launch();
    PQ_HIP(hipMemcpy(out_host, out.p, out.bytes(), hipMemcpyDeviceToHost));
}

}  // namespace pq
