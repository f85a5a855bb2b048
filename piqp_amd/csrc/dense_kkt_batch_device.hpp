// piqp_amd/csrc/dense_kkt_batch_device.hpp -- the per-instance device pieces of the batched dense KKT backend (dense_kkt_batch.hip, whose header holds the table of
// operations), shared with the batched KKTSystem (dense_kktsys_batch.hip), whose kernels iterate on one instance inside one workgroup.  Every piece takes pointers to
// ONE instance's data.  Include only from files compiled with -ffp-contract=off (piqp_amd/build.py, NO_CONTRACT): every fused operation below is an explicit fma().
#pragma once

#include <hip/hip_runtime.h>

#include "dense_factor_batch_device.hpp"

namespace pq {

constexpr int KB_KC = 256;     // K block of syrk_like_lower
constexpr int KB_SLICE = 16;   // columns of GT staged at a time (divides KB_KC)
constexpr int KB_SOLVE_THREADS = 128;
constexpr int KB_EVAL_THREADS = 64;

inline size_t kb_lds_doubles(int n) { return (size_t)n * dfb_ld(n) + (size_t)(KB_SLICE + 1) * n + KB_SLICE; }
inline size_t kb_factor_lds_bytes(int n) { return sizeof(double) * kb_lds_doubles(n) * (n < 32 ? DFB_THREADS / 64 : 1); }
inline size_t kb_solve_lds_bytes(int n) { return sizeof(double) * ((size_t)n * dfb_ld(n) + 3 * (size_t)n + 2); }

// The lower triangle folded into a rectangle of (n + 1) x ceil(n / 2) so that a strided walk over e meets (almost) only elements: column c < ceil(n / 2) of the
// rectangle is column c of the triangle (n - c elements) followed by column n - 1 - c (c + 1 elements).  n odd: the middle column would follow itself; that half
// is skipped (returns false).
__device__ __forceinline__ bool kb_element(int e, int n, int& i, int& j)
{
    const int c = e / (n + 1), r = e % (n + 1);
    if (r < n - c) { j = c; i = c + r; return true; }
    j = n - 1 - c;
    i = j + (r - (n - c));
    return j != c;
}

// The lower triangle of  init + M diag(w) M'  in a[i + j * ld] (LDS), M = n x kdim column-major in global memory.
//   Pu != nullptr: init = P_utri' (+ x_reg on the diagonal, then fma(dinv, ATA, .) when ATA != nullptr);  Pu == nullptr: init = 0.0.
//   w == nullptr: no weights;  recip: the weight is 1.0 / w[k], else w[k].
// dacc[n], gs[KB_SLICE * n], ws[KB_SLICE]: LDS scratch of this instance.  Called by the WHOLE workgroup (barriers); `have` switches an empty slot's work off.  G
// threads per instance, t the thread's index among them.  On return the triangle is complete and a barrier has been passed.  The upper triangle is scratch.
template <int G>
__device__ __forceinline__ void kb_assemble(double* a, double* dacc, double* gs, double* ws, int n, int ld, int kdim, const double* __restrict__ M,
                                            const double* __restrict__ w, bool recip, const double* __restrict__ Pu, const double* __restrict__ x_reg,
                                            const double* __restrict__ ATA, double dinv, bool have, int t)
{
    const int total = (n + 1) * ((n + 1) / 2);
    if (have)
        for (int e = t; e < total; e += G) {
            int i, j;
            if (!kb_element(e, n, i, j)) continue;
            double v = 0.0;
            if (Pu) {
                v = Pu[j + (size_t)i * n];
                if (i == j) v = v + x_reg[j];
                if (ATA) v = fma(dinv, ATA[i + (size_t)j * n], v);
            }
            a[i + j * ld] = v;
        }
    for (int k0 = 0; k0 < kdim; k0 += KB_SLICE) {
        const int kc = kdim - k0 < KB_SLICE ? kdim - k0 : KB_SLICE;
        const bool first = k0 % KB_KC == 0;                                  // the slice opens a K block: acc = 0
        const bool last = k0 + KB_SLICE >= kdim || (k0 + KB_SLICE) % KB_KC == 0;  // the slice closes one: v = v + acc
        __syncthreads();  // (the slice before has been read)
        if (have) {
            const double* src = M + (size_t)k0 * n;
            for (int x = t; x < kc * n; x += G) gs[x] = src[x];
            if (t < kc) ws[t] = w ? (recip ? 1.0 / w[k0 + t] : w[k0 + t]) : 1.0;
        }
        __syncthreads();
        if (have)
            for (int e = t; e < total; e += G) {
                int i, j;
                if (!kb_element(e, n, i, j)) continue;
                double* rest = i == j ? dacc + i : a + j + i * ld;
                double acc = first ? 0.0 : *rest;
                const double* ga = gs + i;
                const double* gb = gs + j;
                if (w) {
                    for (int kk = 0; kk < kc; ++kk) acc = fma(ga[kk * n], 0.0 + ws[kk] * gb[kk * n], acc);  // (0 + b: the micro-kernel's broadcast turns -0 into +0)
                } else {
                    for (int kk = 0; kk < kc; ++kk) acc = fma(ga[kk * n], 0.0 + gb[kk * n], acc);
                }
                if (last) a[i + j * ld] = a[i + j * ld] + acc;
                else *rest = acc;
            }
    }
    __syncthreads();
}

// ---- solve
// the rule of the oracle's vectorised in-order dot products (dense_exact.hip, ex_dot): products rounded on their own, added ascending, only the last of an odd count fused
__device__ __forceinline__ double kb_dot(const double* __restrict__ a, const double* b, int count)
{
    double s = 0.0;
    const int even = count & ~1;
    for (int i = 0; i < even; ++i) s = s + a[i] * b[i];
    if (count & 1) s = fma(a[count - 1], b[count - 1], s);
    return s;
}

// The VECTOR arguments of the helpers below (rhs_*, lhs_*, x) may have been written by the calling launch itself (the refinement loop of dense_kktsys_batch.hip, the
// residuals of dense_solver_batch.hip), so they are plain pointers and must not regain __restrict__: the compiler may serve a const __restrict__ read of a
// workgroup-uniform address from the scalar cache, which does not see vector stores.  The matrices and zinv are never written by a launch that reads them here.

// row i of dense_solve's right-hand side
__device__ __forceinline__ double kb_rhs_row(int i, int n, int p, int m, const double* __restrict__ GT, const double* __restrict__ AT, const double* __restrict__ zinv,
                                             double dinv, const double* rhs_x, const double* rhs_y, const double* rhs_z)
{
    double c = rhs_x[i];
    for (int j = 0; j < m; ++j) c = fma(GT[i + (size_t)j * n], zinv[j] * rhs_z[j], c);
    for (int j = 0; j < p; ++j) c = fma(AT[i + (size_t)j * n], dinv * rhs_y[j], c);
    return c;
}

// solveInPlace of one instance: the factor in a (LDS, leading dimension ld), thread i < n comes with x_i in c; on return xs[0, n) (LDS) holds the solution and a
// barrier has been passed.  pr[2 n], xb[2]: LDS scratch.  Called by the whole workgroup, which has at least n threads.
template <int KIND>
__device__ __forceinline__ void kb_sweeps(const double* a, int n, int ld, double c, double* xs, double* pr, double* xb, int i)
{
    const bool in = i < n;
    for (int j = 0; j < n; ++j) {
        if (i == j) {
            if (KIND == 0) c = c / a[j + j * ld];
            xb[j & 1] = c;
        }
        __syncthreads();
        if (in && i > j) c = fma(-a[i + j * ld], xb[j & 1], c);
    }
    if (in) xs[i] = KIND == 1 ? c / a[i + i * ld] : c;
    __syncthreads();
    for (int j = n - 1; j >= 0; --j) {
        // the products of column j with the values that are final by now (x[j + 1] is not: thread 0 multiplies that one itself)
        if (in && i >= j + 2) pr[(j & 1) * n + i] = a[i + j * ld] * xs[i];
        __syncthreads();
        if (i == 0) {
            const double* col = a + j * ld;
            const double* prod = pr + (j & 1) * n;
            const int count = n - 1 - j, even = count & ~1;
            double s = xs[j];
            if (even > 0) s = s - col[j + 1] * xs[j + 1];
#pragma unroll 8
            for (int q = 1; q < even; ++q) s = s - prod[j + 1 + q];
            if (count & 1) s = fma(-col[n - 1], xs[n - 1], s);
            xs[j] = KIND == 0 ? s / col[j] : s;
        }
    }
    __syncthreads();
}

// lhs_y and lhs_z of dense_solve from the finished lhs_x (x, LDS or global): outputs strided over the `nthreads` threads of the caller
__device__ __forceinline__ void kb_epilogues(int n, int p, int m, const double* __restrict__ GT, const double* __restrict__ AT, const double* __restrict__ zinv,
                                             double dinv, const double* x, const double* rhs_y, const double* rhs_z, double* lhs_y, double* lhs_z, int t, int nthreads)
{
    for (int j = t; j < p; j += nthreads) {
        const double s = kb_dot(AT + (size_t)j * n, x, n);
        double v = dinv * s;
        v = fma(-dinv, rhs_y[j], v);
        lhs_y[j] = v;
    }
    for (int j = t; j < m; j += nthreads) {
        const double s = kb_dot(GT + (size_t)j * n, x, n);
        double v = 1.0 * s;
        v = v - rhs_z[j];
        v = v * zinv[j];
        lhs_z[j] = v;
    }
}

// ---- evaluators
// dense_eval_P_x (k_ex_eval_P): z[t] is touched first by column t:  z[t] = 0 + fma(P_tt, alpha x_t, alpha * s_t),  s_t the dot product over the part of column t above
// the diagonal;  after that by every column j > t:  z[t] = fma(P_tj, alpha x_j, z[t])
__device__ __forceinline__ double kb_eval_P_row(int t, int n, const double* __restrict__ Pu, double alpha, const double* x)
{
    const double* col = Pu + (size_t)t * n;
    const double s = kb_dot(col, x, t);
    double v = 0.0 + fma(col[t], alpha * x[t], alpha * s);
    for (int j = t + 1; j < n; ++j) v = fma(Pu[t + (size_t)j * n], alpha * x[j], v);
    return v;
}
// gemv_t (k_ex_gemv_t mode 0): alpha * dot(column j, x)
__device__ __forceinline__ double kb_gemv_t_col(int j, int rows, const double* __restrict__ M, const double* x, double alpha)
{
    return alpha * kb_dot(M + (size_t)j * rows, x, rows);
}
// gemv_n into a zeroed vector (k_ex_gemv_n): the chain over ascending j of fma(M[i][j], alpha * x[j], .)
__device__ __forceinline__ double kb_gemv_n_row(int i, int rows, int cols, const double* __restrict__ M, const double* x, double alpha)
{
    double c = 0.0;
    for (int j = 0; j < cols; ++j) c = fma(M[i + (size_t)j * rows], alpha * x[j], c);
    return c;
}

// ---- the finite-bound tables of the layers above the backend (dense_kktsys_batch.hip, dense_solver_batch.hip).  A row of tables is
//   has_l[m], has_u[m] (the position of row i of G in h_l_idx / h_u_idx, or -1), pos_l[n], pos_u[n] (the same for the box lists; the KKT system only), x_l_idx, x_u_idx.
// Shared sets: ONE row for the whole batch; the six pointers and the four counts are what the kernels had as plain arguments before sets per instance existed, and a
// kernel built with PER = false uses them as they are: nothing is computed and nothing is read per instance, the code is the one of before.
// Sets per instance (PER = true): the six pointers are those of instance 0's row, row `inst` lies inst * stride ints further, and the instance's counts are
// cnt[4 inst ..] = n_h_l, n_h_u, n_x_l, n_x_u.
struct KbBounds {
    const int *has_l, *has_u, *pos_l, *pos_u, *xl_idx, *xu_idx;
    int nhl, nhu, nxl, nxu;
    const int* cnt;
    int stride;
};
template <bool PER>
__device__ __forceinline__ KbBounds kb_bound_row(const KbBounds& B, long long inst)
{
    if (!PER) return B;
    KbBounds r = B;
    const size_t off = (size_t)inst * B.stride;
    r.has_l += off; r.has_u += off; r.pos_l += off; r.pos_u += off; r.xl_idx += off; r.xu_idx += off;
    const int* c = B.cnt + 4 * (size_t)inst;
    r.nhl = c[0]; r.nhu = c[1]; r.nxl = c[2]; r.nxu = c[3];
    return r;
}

// ---- clone by a list of instances (pq_*_batch_clone_select of the three layers): row j of dst is row idx[j] of src, rows of wpr words of W -- uint4, unsigned
// long long or unsigned, the widest that divides the row's bytes and both bases (kb_gather_rows, dense_kkt_batch_internal.hpp).  A copy of bits: a word is loaded and
// stored, nothing is computed on it.  Rows of 256 words and more: a workgroup moves one chunk of 1024 words of one row per step, consecutive lanes consecutive words
// (16 KiB with uint4; the 128 KiB row of Pu at n = 128 is 8 chunks).  Shorter rows: a workgroup moves 256 / wpr whole rows per step, lane t word t % wpr of row
// t / wpr, so the lanes of a row still read consecutive words (a row of one word: 256 rows per step).  The row index comes from blockIdx.x and a grid-stride loop and
// is held in 64 bits, as is every offset; idx has been checked against the source's batch on the host.
constexpr int KB_GATHER_THREADS = 256;
constexpr int KB_GATHER_CHUNK = 4 * KB_GATHER_THREADS;
constexpr int KB_GATHER_MAX_GRID = 8192;
template <class W>
__global__ __launch_bounds__(KB_GATHER_THREADS) void k_kb_gather_rows(W* __restrict__ dst, const W* __restrict__ src, const int* __restrict__ idx, size_t count,
                                                                      size_t wpr)
{
    const unsigned t = threadIdx.x;
    if (wpr >= (size_t)KB_GATHER_THREADS) {
        const size_t cpr = (wpr + KB_GATHER_CHUNK - 1) / KB_GATHER_CHUNK, units = count * cpr;
        for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
            const size_t row = u / cpr, w0 = (u % cpr) * KB_GATHER_CHUNK;
            const size_t w1 = w0 + KB_GATHER_CHUNK < wpr ? w0 + KB_GATHER_CHUNK : wpr;
            const W* s = src + (size_t)idx[row] * wpr;
            W* d = dst + row * wpr;
            for (size_t w = w0 + t; w < w1; w += KB_GATHER_THREADS) d[w] = s[w];
        }
        return;
    }
    const unsigned len = (unsigned)wpr, rpb = KB_GATHER_THREADS / len, r = t / len, w = t % len;
    if (r >= rpb) return;  // (the lanes past the last whole row; no barrier below)
    const size_t groups = (count + rpb - 1) / rpb;
    for (size_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const size_t row = g * rpb + r;
        if (row < count) dst[row * wpr + w] = src[(size_t)idx[row] * wpr + w];
    }
}

// ---- the mirror, for the calls that act on a list of instances in place (pq_solver_batch_*_select): row idx[j] of dst is row j of src -- or, with same_row, row
// idx[j] of src: the listed rows of one [batch][len] array into another.  The same word-width rule (kb_scatter_rows), the same two walks, a copy of bits.  The
// entries of idx are distinct (checked on the host), so no two rows of a launch write the same place.
template <class W>
__global__ __launch_bounds__(KB_GATHER_THREADS) void k_kb_scatter_rows(W* __restrict__ dst, const W* __restrict__ src, const int* __restrict__ idx, size_t count,
                                                                       size_t wpr, int same_row)
{
    const unsigned t = threadIdx.x;
    if (wpr >= (size_t)KB_GATHER_THREADS) {
        const size_t cpr = (wpr + KB_GATHER_CHUNK - 1) / KB_GATHER_CHUNK, units = count * cpr;
        for (size_t u = blockIdx.x; u < units; u += gridDim.x) {
            const size_t row = u / cpr, w0 = (u % cpr) * KB_GATHER_CHUNK;
            const size_t w1 = w0 + KB_GATHER_CHUNK < wpr ? w0 + KB_GATHER_CHUNK : wpr;
            const size_t to = (size_t)idx[row];
            const W* s = src + (same_row ? to : row) * wpr;
            W* d = dst + to * wpr;
            for (size_t w = w0 + t; w < w1; w += KB_GATHER_THREADS) d[w] = s[w];
        }
        return;
    }
    const unsigned len = (unsigned)wpr, rpb = KB_GATHER_THREADS / len, r = t / len, w = t % len;
    if (r >= rpb) return;  // (the lanes past the last whole row; no barrier below)
    const size_t groups = (count + rpb - 1) / rpb;
    for (size_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const size_t row = g * rpb + r;
        if (row < count) {
            const size_t to = (size_t)idx[row];
            dst[to * wpr + w] = src[(same_row ? to : row) * wpr + w];
        }
    }
}

}  // namespace pq
