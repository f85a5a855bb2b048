// piqp_amd/csrc/ingest_kernels.hpp -- problem data that already lives in HBM, brought into the layouts the solvers store (ingest_kernels.hip).
// Nothing here computes: copies, a transpose, a triangle mask, a mapped gather and a zero-fill, so a device-fed solver holds bit for bit what a host-fed one uploads.
#pragma once

#include "common.hpp"

namespace pq {

// dst (column-major cols x rows, leading dimension cols) = transpose of src (column-major rows x cols, leading dimension rows); both device, distinct.
// upper_only (rows == cols): only the entries of dst on or above its diagonal are taken from src, the rest of dst is written as zero and the
// corresponding entries of src are never loaded.
void ingest_transpose(double* dst, const double* src, int rows, int cols, bool upper_only, hipStream_t st);
// dst = upper triangle of the column-major n x n src, zeros strictly below the diagonal (those entries of src are never loaded)
void ingest_copy_upper(double* dst, const double* src, int n, hipStream_t st);
// sparse problems: dst[q] = src[src_idx[q]] for q < count (all device; src_idx built on the host from the sparsity patterns, every entry inside src)
void ingest_gather(double* dst, const double* src, const int* src_idx, int count, hipStream_t st);
// vals[colptr[c] .. colptr[c + 1]) = 0 for each of the ncols listed columns c (all device): the rows of G without a finite bound, in the stored G^T
void ingest_zero_columns(double* vals, const int* colptr, const int* cols, int ncols, hipStream_t st);
// *flag |= 1 if any v[q * len + i] (q < batch) is finite on its side (lower: v > -1e30, upper: v < 1e30) where finite[i] == 0, or the reverse
void ingest_check_finite_pattern(const double* v, const int* finite, int batch, int len, bool lower, int* flag, hipStream_t st);
// measurement: read + write GB/s of ingest_transpose on a rows x cols matrix (pq_microbench_transpose)
double microbench_transpose(int rows, int cols, int iters, hipStream_t st);

}  // namespace pq
