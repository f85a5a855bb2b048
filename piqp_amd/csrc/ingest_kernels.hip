// piqp_amd/csrc/ingest_kernels.hip -- see ingest_kernels.hpp.  DenseSolver::setup / update take P (n x n), A (p x n), G (m x n) in either storage order and
// keep upper(P), A^T, G^T column-major (solver.hpp:169-192); when the caller's matrices are in HBM these kernels do what make_dense_host_data and
// Solver::update_dense do with host loops.  A row-major A IS the column-major A^T (plain copy, no kernel); what remains is an out-of-place transpose and a
// triangle mask.
#include "ingest_kernels.hpp"

namespace pq {

namespace {

// One 64 x 64 tile per workgroup of 256 threads (4 waves); the grid covers the matrix.  Both global sides are coalesced: a wave reads 64 consecutive doubles
// of one source column (512 B) and writes 64 consecutive doubles of one destination column.  The tile goes through LDS with rows of 65 doubles: the store
// tile[k][lane] walks consecutive addresses; the transposed load tile[lane][k] has a lane stride of 65 doubles = 130 dwords, i.e. bank (2 lane) mod 64 of
// the 64 four-byte banks -- the 32 lanes of a half-wave (the conflict group of an 8-byte LDS read) land on 32 distinct bank pairs.  A row of 64 (or 66, 68)
// doubles would put them on 1 (2, 4) pairs.
constexpr int TILE = 64, TILE_LD = TILE + 1, TP_THREADS = 256, TP_WAVES = TP_THREADS / 64;

// dst[c + r * cols] = src[r + c * rows].  UPPER (rows == cols): dst(c, r) with c > r is zero and src is not read there.
template <bool UPPER>
__global__ __launch_bounds__(TP_THREADS) void k_ingest_transpose(double* __restrict__ dst, const double* __restrict__ src, int rows, int cols)
{
    __shared__ double tile[TILE][TILE_LD];
    const int r0 = blockIdx.x * TILE, c0 = blockIdx.y * TILE, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // the tile of dst holds rows c0 .. c0 + 63 and columns r0 .. r0 + 63: entirely below the diagonal when c0 > r0
    const bool below = UPPER && blockIdx.y > blockIdx.x;
    if (!below) {
        const int r = r0 + lane;
        for (int k = w; k < TILE; k += TP_WAVES) {
            const int c = c0 + k;
            if (r < rows && c < cols && !(UPPER && c > r)) tile[k][lane] = src[(size_t)c * rows + r];
        }
    }
    __syncthreads();
    const int c = c0 + lane;
    for (int k = w; k < TILE; k += TP_WAVES) {
        const int r = r0 + k;
        if (r >= rows || c >= cols) continue;
        double v = 0.0;
        if (!below && !(UPPER && c > r)) v = tile[lane][k];  // exactly the entries the loop above stored
        dst[(size_t)r * cols + c] = v;
    }
}

// dst = upper(src), column-major n x n: one workgroup per 256 rows of a column, columns strided over gridDim.y
__global__ __launch_bounds__(256) void k_ingest_copy_upper(double* __restrict__ dst, const double* __restrict__ src, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int j = blockIdx.y; j < n; j += gridDim.y) dst[(size_t)j * n + i] = i <= j ? src[(size_t)j * n + i] : 0.0;
}

// grid: x over the entries of a vector, y strided over the instances
__global__ __launch_bounds__(256) void k_ingest_check_finite_pattern(const double* __restrict__ v, const int* __restrict__ finite, int batch, int len, int lower,
                                                                     int* __restrict__ flag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const bool fin = finite[i] != 0;
    bool bad = false;
    for (int q = blockIdx.y; q < batch; q += gridDim.y) {
        const double x = v[(size_t)q * len + i];
        bad |= (lower ? x > -1e30 : x < 1e30) != fin;
    }
    if (bad) atomicOr(flag, 1);
}

// ---- sparse problems: the caller's CSC value arrays -> the stored order of upper(P), A^T, G^T (SparseSolver::setup / update, solver.hpp:169-192,317-358).  The
// index work is done once on the host (gather maps, Solver setup); per call only values move: one 8-byte load through a 4-byte index and one coalesced 8-byte store
// per stored entry, plain vector memory instructions.
// dst[q] = src[src_idx[q]], q < count.  Entries of src no map entry names (the strictly lower triangle of a full P) are never loaded.
__global__ __launch_bounds__(256) void k_ingest_gather(double* __restrict__ dst, const double* __restrict__ src, const int* __restrict__ src_idx, int count)
{
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < count; q += (long long)gridDim.x * 256) dst[q] = src[src_idx[q]];  // (64-bit: q + stride may pass 2^31)
}
// vals[colptr[c] .. colptr[c + 1]) = 0 for the listed columns c of a CSC matrix (G^T: column c is row c of G); one workgroup per listed column
__global__ __launch_bounds__(256) void k_ingest_zero_columns(double* __restrict__ vals, const int* __restrict__ colptr, const int* __restrict__ cols, int ncols)
{
    for (int k = blockIdx.x; k < ncols; k += gridDim.x) {
        const int c = cols[k], hi = colptr[c + 1];
        for (int q = colptr[c] + threadIdx.x; q < hi; q += 256) vals[q] = 0.0;
    }
}

}  // namespace

void ingest_gather(double* dst, const double* src, const int* src_idx, int count, hipStream_t st)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_ingest_gather, dim3(std::min(div_up(count, 256), 65536)), dim3(256), 0, st, dst, src, src_idx, count);
    PQ_HIP(hipGetLastError());
}

void ingest_zero_columns(double* vals, const int* colptr, const int* cols, int ncols, hipStream_t st)
{
    if (ncols <= 0) return;
    hipLaunchKernelGGL(k_ingest_zero_columns, dim3(std::min(ncols, 65536)), dim3(256), 0, st, vals, colptr, cols, ncols);
    PQ_HIP(hipGetLastError());
}

void ingest_transpose(double* dst, const double* src, int rows, int cols, bool upper_only, hipStream_t st)
{
    if (rows <= 0 || cols <= 0) return;
    if (upper_only && rows != cols) throw std::runtime_error("ingest_transpose: the triangle mask needs a square matrix");
    const dim3 grid(div_up(rows, TILE), div_up(cols, TILE));
    if (grid.y > 65535u) throw std::runtime_error("ingest_transpose: matrix too wide");
    if (upper_only) hipLaunchKernelGGL(k_ingest_transpose<true>, grid, dim3(TP_THREADS), 0, st, dst, src, rows, cols);
    else hipLaunchKernelGGL(k_ingest_transpose<false>, grid, dim3(TP_THREADS), 0, st, dst, src, rows, cols);
    PQ_HIP(hipGetLastError());
}

void ingest_copy_upper(double* dst, const double* src, int n, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ingest_copy_upper, dim3(div_up(n, 256), std::min(n, 65535)), dim3(256), 0, st, dst, src, n);
    PQ_HIP(hipGetLastError());
}

void ingest_check_finite_pattern(const double* v, const int* finite, int batch, int len, bool lower, int* flag, hipStream_t st)
{
    if (batch <= 0 || len <= 0) return;
    hipLaunchKernelGGL(k_ingest_check_finite_pattern, dim3(div_up(len, 256), std::min(batch, 1024)), dim3(256), 0, st, v, finite, batch, len, lower ? 1 : 0, flag);
    PQ_HIP(hipGetLastError());
}

// read + write bytes per second of the transpose of a rows x cols matrix, as pq_microbench_hbm_copy counts them
double microbench_transpose(int rows, int cols, int iters, hipStream_t s)
{
    const size_t cnt = (size_t)rows * cols;
    DBuf<double> a(cnt), b(cnt);
    PQ_HIP(hipMemsetAsync(a.p, 1, cnt * sizeof(double), s));
    Event e0(0), e1(0);
    ingest_transpose(b.p, a.p, rows, cols, false, s);
    stream_wait(s);
    PQ_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) ingest_transpose(b.p, a.p, rows, cols, false, s);
    PQ_HIP(hipEventRecord(e1, s));
    PQ_HIP(hipEventSynchronize(e1));
    float ms = 0;
    PQ_HIP(hipEventElapsedTime(&ms, e0, e1));
    return 2.0 * (double)cnt * sizeof(double) * iters / (ms * 1e-3) * 1e-9;
}

}  // namespace pq
