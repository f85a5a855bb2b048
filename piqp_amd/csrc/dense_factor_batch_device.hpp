// piqp_amd/csrc/dense_factor_batch_device.hpp -- the in-LDS right-looking factorisation of dense_factor_batch.hip as a device function, shared by k_dfb_factor
// (pq_dense_factor_batch_*: the matrix is loaded from memory) and k_kb_factor (dense_kkt_batch.hip, pq_kkt_batch_*: the matrix is assembled in LDS).  The table of
// operations and the launch shape are in the header of dense_factor_batch.hip.  Include only from files compiled with -ffp-contract=off (piqp_amd/build.py,
// NO_CONTRACT): every fused operation below is an explicit fma().
#pragma once

#include <hip/hip_runtime.h>

namespace pq {

constexpr int DFB_THREADS = 256;

// dense/ldlt_no_pivot.hpp:321-323 == Eigen LLT.h blocked()
inline int dfb_block_size_rule(int size)
{
    int bs = size / 8;
    bs = (bs / 16) * 16;
    if (bs < 8) bs = 8;
    if (bs > 128) bs = 128;
    return bs;
}

inline int dfb_ld(int n) { return n | 1; }

// Factors the matrix whose lower triangle lies in a[i + j * ld] (LDS) in place.  KIND 0: Eigen::LLT, 1: LDLTNoPivot (the upper triangle of the square is its
// workspace).  G: threads per matrix (256: one matrix per workgroup, 64: four); g: the matrix's slot in the workgroup, t: the thread's index within the G.
// width: n below 32 (unblocked), dfb_block_size_rule(n) above.  s_fail[g] must be -1 and the matrix complete (a workgroup barrier passed) on entry; on return
// s_fail[g] is -1 or the failing column.  Called by the WHOLE workgroup (it contains workgroup barriers); `have` switches the work of an empty slot off.
// Returns whether the matrix factored.
template <int KIND, int G>
__device__ __forceinline__ bool dfb_factor_in_lds(double* a, int n, int ld, int width, bool have, int g, int t, int* s_fail)
{
    bool live = have;
    for (int k = 0; k < n && (G != DFB_THREADS || live); k += width) {
        const int bs = n - k < width ? n - k : width;
        const int rs = n - k - bs;
        // ---- the diagonal block, column by column: thread t owns row k + t
        for (int kc = 0; kc < bs; ++kc) {
            const int c = k + kc;
            double v = 0.0;
            if (live && t == kc) {
                if (KIND == 0) {
                    double x = a[c + c * ld];
                    if (kc > 0) {
                        double s = 0.0;
                        for (int j = k; j < c; ++j) { const double w = a[c + j * ld]; s = fma(w, w, s); }
                        x = x - s;
                    }
                    if (!(x > 0.0)) s_fail[g] = c;
                    else a[c + c * ld] = sqrt(x);
                } else {
                    if (kc > 0) {
                        double s = 0.0;
                        for (int j = k; j < c; ++j) { const double w = a[c + j * ld]; const double tj = a[j + j * ld] * w; s = fma(w, tj, s); }
                        a[c + c * ld] = a[c + c * ld] - s;
                    }
                    if (a[c + c * ld] == 0.0) s_fail[g] = c;
                }
            } else if (live && t > kc && t < bs) {
                const int i = k + t;
                v = a[i + c * ld];
                if (KIND == 0) {
                    for (int j = k; j < c; ++j) v = fma(-a[i + j * ld], a[c + j * ld], v);
                } else {
                    for (int j = k; j < c; ++j) { const double tj = a[j + j * ld] * a[c + j * ld]; v = fma(-a[i + j * ld], tj, v); }
                }
            }
            __syncthreads();
            live = have && s_fail[g] < 0;
            if (G == DFB_THREADS && !live) break;  // (one matrix per workgroup: the same answer in every thread)
            if (live && t > kc && t < bs) a[(k + t) + c * ld] = v / a[c + c * ld];
            __syncthreads();
        }
        if (G == DFB_THREADS && !live) break;
        if (rs <= 0) continue;
        // ---- A21 <- A21 L11^-T (LLT) resp. A21 (L11^T unit-upper)^-1 D11^-1, and t = A21 D11: one thread per row
        if (live)
            for (int r = k + bs + t; r < n; r += G) {
                for (int j = 0; j < bs; ++j) {
                    double x = a[r + (k + j) * ld];
                    for (int kk = 0; kk < j; ++kk) x = fma(-a[r + (k + kk) * ld], a[(k + j) + (k + kk) * ld], x);
                    if (KIND == 0) x = x / a[(k + j) + (k + j) * ld];
                    a[r + (k + j) * ld] = x;
                }
                if (KIND == 1)
                    for (int j = 0; j < bs; ++j) {
                        const double d = a[(k + j) + (k + j) * ld];
                        const double dinv = 1.0 / d;
                        const double col = a[r + (k + j) * ld] * dinv;
                        a[r + (k + j) * ld] = col;
                        a[(k + j) + r * ld] = col * d;  // t, in the upper triangle
                    }
            }
        __syncthreads();
        // ---- A22_L -= a A21^T: one row and four columns per thread
        if (live) {
            const int nq = (rs + 3) / 4;
            for (int e = t; e < rs * nq; e += G) {
                const int ii = e % rs, jq = (e / rs) * 4;
                if (jq > ii) continue;
                const int i = k + bs + ii;
                int jc[4];
                for (int q = 0; q < 4; ++q) jc[q] = k + bs + (jq + q <= ii ? jq + q : jq);
                double acc[4] = {0.0, 0.0, 0.0, 0.0};
                for (int kk = 0; kk < bs; ++kk) {
                    const double av = KIND == 0 ? a[i + (k + kk) * ld] : a[(k + kk) + i * ld];
                    for (int q = 0; q < 4; ++q) acc[q] = fma(av, 0.0 + a[jc[q] + (k + kk) * ld], acc[q]);  // (0 + b: the micro-kernel's broadcast)
                }
                for (int q = 0; q < 4; ++q)
                    if (jq + q <= ii) a[i + jc[q] * ld] = a[i + jc[q] * ld] - acc[q];
            }
        }
        __syncthreads();
    }
    return live;
}

}  // namespace pq
