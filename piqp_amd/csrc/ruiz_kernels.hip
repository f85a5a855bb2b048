// piqp_amd/csrc/ruiz_kernels.hip -- device Ruiz equilibration (see ruiz_device.hpp).  HBM-bound byte pushing: no matrix cores here.
#include "ruiz_device.hpp"
#include "ingest_kernels.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "solver.hpp"

namespace pq {
namespace {

__device__ __forceinline__ double limit_scaling(double d) { return d < 1e-4 ? 1.0 : (d > 1e4 ? 1e4 : d); }  // dense/preconditioner.hpp:513-523
__device__ __forceinline__ double inv_sqrt_limited(double d) { return 1.0 / sqrt(limit_scaling(d)); }
// max of non-negative doubles as an integer max of their bit patterns: exact and order independent
__device__ __forceinline__ void amax(double* a, double v)
{
    if (v > 0.0) atomicMax(reinterpret_cast<unsigned long long*>(a), (unsigned long long)__double_as_longlong(v));
}
__device__ __forceinline__ void amax_lds(double* a, double v)
{
    if (v > 0.0) atomicMax(reinterpret_cast<unsigned long long*>(a), (unsigned long long)__double_as_longlong(v));
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// the value of `v` maximised over the workgroup, returned to every thread (red: 16 doubles of LDS)
__device__ __forceinline__ double block_max(double v, double* red)
{
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < (int)(blockDim.x + 63) / 64; ++w) r = fmax(r, red[w]);
    return r;
}
// workgroup barrier that also orders plain accesses against the L2 atomics of other waves (vector L1 is not coherent with them)
__device__ __forceinline__ void sync_mem()
{
    __threadfence();
    __syncthreads();
    __threadfence();
}

// ------------------------------------------------------------------------------------------------ sparse, one workgroup per instance
// inf-norms of the columns of the symmetric matrix stored as the upper triangle (Px): out[k] (zeroed by the caller) via atomic max
__device__ __forceinline__ void sym_col_norms(int n, const int* __restrict__ Pp, const int* __restrict__ Pi, const double* Px, double* out, int t0, int nt)
{
    for (int j = t0; j < n; j += nt) {
        double cm = 0.0;
        for (int q = Pp[j]; q < Pp[j + 1]; ++q) {
            const int r = Pi[q];
            const double a = fabs(Px[q]);
            cm = fmax(cm, a);
            if (r != j) amax(out + r, a);
        }
        amax(out + j, cm);
    }
}
// inf-norms of the rows (-> rown, atomic) and the columns (-> coln, plain store) of a CSC matrix
__device__ __forceinline__ void rows_and_cols(int cols, const int* __restrict__ Tp, const int* __restrict__ Ti, const double* Tx, double* rown, double* coln, int t0, int nt)
{
    for (int j = t0; j < cols; j += nt) {
        double cm = 0.0;
        for (int q = Tp[j]; q < Tp[j + 1]; ++q) {
            const double a = fabs(Tx[q]);
            cm = fmax(cm, a);
            amax(rown + Ti[q], a);
        }
        coln[j] = cm;
    }
}
// sparse/utils.hpp:172-199 order: rows first, then columns; `pre` multiplies first when USE_PRE (scale_P_scalar before scale_P)
template <bool USE_PRE>
__device__ __forceinline__ void scale_csc(int cols, const int* __restrict__ Tp, const int* __restrict__ Ti, double* Tx, const double* srow, const double* scol, double pre, int t0, int nt)
{
    for (int j = t0; j < cols; j += nt) {
        const double sc = scol[j];
        for (int q = Tp[j]; q < Tp[j + 1]; ++q) {
            double v = Tx[q];
            if (USE_PRE) v *= pre;
            Tx[q] = (v * srow[Ti[q]]) * sc;
        }
    }
}

// GRID = false: one workgroup per instance (the batched solver; a single small QP).  GRID = true (round 4): the gridDim.x workgroups of the launch share ONE
// instance -- every loop strides over the whole grid, the workgroup barriers become grid barriers (a monotonic counter in a.grid_ws; all workgroups are
// resident: the launch has at most one per CU), the two maxima are reduced through one slot per iteration.  The statements, and the order of the one sum that
// has an order (the mean of the column norms, thread 0 of workgroup 0), are the same: bitwise the same scaling.  One workgroup needed 13 ms for the C3 pattern.
template <bool GRID>
__device__ __forceinline__ void ruiz_sync(unsigned long long* ws, unsigned& epoch)
{
    if constexpr (!GRID) { sync_mem(); return; }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        epoch += gridDim.x;
        unsigned* cnt = reinterpret_cast<unsigned*>(ws);
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        while (__hip_atomic_load(cnt, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < epoch) __builtin_amdgcn_s_sleep(2);
    }
    __syncthreads();
    __threadfence();
}
// maximum over all threads that share the instance, returned to every thread; slot: a zero-initialised word of a.grid_ws used once
template <bool GRID>
__device__ __forceinline__ double ruiz_max(double v, double* red, unsigned long long* ws, int slot, unsigned& epoch)
{
    v = block_max(v, red);
    if constexpr (!GRID) return v;
    if (threadIdx.x == 0) amax(reinterpret_cast<double*>(ws + slot), v);
    ruiz_sync<GRID>(ws, epoch);
    return __longlong_as_double((long long)__hip_atomic_load(ws + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
constexpr int RUIZ_WS_DEV = 2, RUIZ_WS_CINF = 66, RUIZ_WS_GSUM = 130, RUIZ_WS_WORDS = 132;  // counter | per-iteration maxima (<= 64 iterations) | the mean's sum

template <bool GRID>
__global__ void k_ruiz_sparse(RuizSparseArgs a)
{
    __shared__ double red[16];
    __shared__ double gsum;
    const int inst = GRID ? 0 : (a.inst_list ? a.inst_list[blockIdx.x] : (int)blockIdx.x);
    const long long o = (long long)inst * a.stride;
    const int n = a.n, p = a.p, m = a.m, N = n + p + m;
    const int t = GRID ? (int)(blockIdx.x * blockDim.x + threadIdx.x) : (int)threadIdx.x, NT = GRID ? (int)(gridDim.x * blockDim.x) : (int)blockDim.x;
    unsigned long long* ws = a.grid_ws;
    unsigned epoch = 0;
    double *Px = a.Px + o, *ATx = a.ATx + o, *GTx = a.GTx + o, *c = a.c + o, *xbs = a.xbs + o;
    double *delta = a.delta + o, *delta_b = a.delta_b + o, *di = a.delta_inv + o, *dib = a.delta_b_inv + o, *tmp = a.tmp + o;
    const double *s = delta, *sb = delta_b;  // what the tail multiplies with
    if (a.mode == RUIZ_COMPUTE) {
        // sparse/preconditioner.hpp:65-206.  di / dib (the inverse slots, rewritten at the end) hold the scaling of the current pass.
        double cs = 1.0;
        for (int i = t; i < N; i += NT) { delta[i] = 1.0; di[i] = 0.0; }
        for (int i = t; i < n; i += NT) { delta_b[i] = 1.0; dib[i] = 0.0; }
        ruiz_sync<GRID>(ws, epoch);
        for (int it = 0; it < a.max_iter; ++it) {
            double dev = 0.0;
            for (int i = t; i < N; i += NT) dev = fmax(dev, fabs(1.0 - di[i]));
            for (int i = t; i < n; i += NT) dev = fmax(dev, fabs(1.0 - dib[i]));
            dev = ruiz_max<GRID>(dev, red, ws, RUIZ_WS_DEV + it, epoch);
            if (!(dev > a.eps)) break;
            for (int i = t; i < N; i += NT) di[i] = 0.0;
            ruiz_sync<GRID>(ws, epoch);
            sym_col_norms(n, a.Pp, a.Pi, Px, di, t, NT);
            if (p > 0) rows_and_cols(p, a.ATp, a.ATi, ATx, di, di + n, t, NT);
            if (m > 0) rows_and_cols(m, a.GTp, a.GTi, GTx, di, di + n + p, t, NT);
            ruiz_sync<GRID>(ws, epoch);
            for (int i = t; i < N; i += NT) {
                if (i < n) {
                    const double xb = xbs[i];
                    di[i] = inv_sqrt_limited(fmax(di[i], xb));
                    dib[i] = inv_sqrt_limited(xb);
                } else {
                    di[i] = inv_sqrt_limited(di[i]);
                }
            }
            ruiz_sync<GRID>(ws, epoch);
            scale_csc<false>(n, a.Pp, a.Pi, Px, di, di, 1.0, t, NT);
            for (int i = t; i < n; i += NT) c[i] *= di[i];
            if (p > 0) scale_csc<false>(p, a.ATp, a.ATi, ATx, di, di + n, 1.0, t, NT);
            if (m > 0) scale_csc<false>(m, a.GTp, a.GTi, GTx, di, di + n + p, 1.0, t, NT);
            for (int i = t; i < n; i += NT) { xbs[i] *= dib[i] * di[i]; delta_b[i] *= dib[i]; }
            for (int i = t; i < N; i += NT) delta[i] *= di[i];
            if (a.scale_cost) {
                for (int i = t; i < n; i += NT) tmp[i] = 0.0;
                ruiz_sync<GRID>(ws, epoch);
                sym_col_norms(n, a.Pp, a.Pi, Px, tmp, t, NT);
                ruiz_sync<GRID>(ws, epoch);
                if (t == 0) {
                    double g = 0.0;
                    for (int k = 0; k < n; ++k) g += tmp[k];
                    if constexpr (GRID) __hip_atomic_store(reinterpret_cast<double*>(ws + RUIZ_WS_GSUM), g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else gsum = g;
                }
                double cinf = 0.0;
                for (int i = t; i < n; i += NT) cinf = fmax(cinf, fabs(c[i]));
                cinf = ruiz_max<GRID>(cinf, red, ws, RUIZ_WS_CINF + it, epoch);  // (its barriers also publish gsum)
                double gamma = (GRID ? __hip_atomic_load(reinterpret_cast<double*>(ws + RUIZ_WS_GSUM), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : gsum) / (double)n;
                gamma = limit_scaling(gamma);
                gamma = limit_scaling(fmax(gamma, cinf));
                gamma = 1.0 / gamma;
                for (int j = t; j < n; j += NT) for (int q = a.Pp[j]; q < a.Pp[j + 1]; ++q) Px[q] *= gamma;
                for (int i = t; i < n; i += NT) c[i] *= gamma;
                cs *= gamma;
            }
            ruiz_sync<GRID>(ws, epoch);
        }
        ruiz_sync<GRID>(ws, epoch);
        for (int i = t; i < N; i += NT) di[i] = 1.0 / delta[i];
        for (int i = t; i < n; i += NT) dib[i] = 1.0 / delta_b[i];
        if (t == 0) a.c_scale[inst] = cs;
        ruiz_sync<GRID>(ws, epoch);
    } else {
        // scale_data with reuse_prev_scaling (:207-217) / unscale_data (:224-258): the same products with (c, delta) or their inverses
        double cs = a.c_scale[inst];
        if (a.mode == RUIZ_UNSCALE) { cs = 1.0 / cs; s = di; sb = dib; }
        scale_csc<true>(n, a.Pp, a.Pi, Px, s, s, cs, t, NT);
        for (int i = t; i < n; i += NT) c[i] *= cs * s[i];
        if (p > 0) scale_csc<false>(p, a.ATp, a.ATi, ATx, s, s + n, 1.0, t, NT);
        if (m > 0) scale_csc<false>(m, a.GTp, a.GTi, GTx, s, s + n + p, 1.0, t, NT);
        for (int i = t; i < n; i += NT) xbs[i] *= sb[i] * s[i];
    }
    if (a.b) for (int i = t; i < p; i += NT) a.b[o + i] *= s[n + i];
    if (a.h_l) for (int i = t; i < m; i += NT) a.h_l[o + i] *= s[n + p + i];
    if (a.h_u) for (int i = t; i < m; i += NT) a.h_u[o + i] *= s[n + p + i];
    const int* row = (!GRID && a.lists) ? a.lists + (long long)inst * a.lists_stride : nullptr;
    const int n_x_l = row ? row[2] : a.n_x_l, n_x_u = row ? row[3] : a.n_x_u;
    const int *x_l_idx = row ? row + a.lists_x_l : a.x_l_idx, *x_u_idx = row ? row + a.lists_x_u : a.x_u_idx;
    if (a.x_l) for (int k = t; k < n_x_l; k += NT) a.x_l[o + k] *= sb[x_l_idx[k]];
    if (a.x_u) for (int k = t; k < n_x_u; k += NT) a.x_u[o + k] *= sb[x_u_idx[k]];
}

// ------------------------------------------------------------------------------------------------ dense, tiled
constexpr int TR = 256, TC = 32;  // tile = 256 rows (one per thread, coalesced along the column) x 32 columns

struct DenseState {  // device-resident control block of one equilibration
    double c, c_inv, gamma;
    int done;
};

__global__ void k_rzd_begin(int N, int n, double* delta, double* delta_b, double* di, double* dib, DenseState* st)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) { delta[i] = 1.0; di[i] = 0.0; }
    if (i < n) { delta_b[i] = 1.0; dib[i] = 0.0; }
    if (i == 0) { st->c = 1.0; st->gamma = 1.0; st->done = 0; }
}
// head of one pass: converged? (dense/preconditioner.hpp:82) -- otherwise clear the norm accumulators
__global__ void k_rzd_check(int N, int n, double* di, const double* dib, double* tmp, double eps, DenseState* st)
{
    __shared__ double red[16];
    if (st->done) return;
    double dev = 0.0;
    for (int i = threadIdx.x; i < N; i += blockDim.x) dev = fmax(dev, fabs(1.0 - di[i]));
    for (int i = threadIdx.x; i < n; i += blockDim.x) dev = fmax(dev, fabs(1.0 - dib[i]));
    dev = block_max(dev, red);
    if (!(dev > eps)) { if (threadIdx.x == 0) st->done = 1; return; }
    for (int i = threadIdx.x; i < N; i += blockDim.x) di[i] = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) tmp[i] = 0.0;
}
// One pass over a column-major rows x cols matrix, tile by tile: optional scalar factor (USE_PRE: M *= *pre_ptr, scale_P_scalar), optional
// row / column scaling (VEC), optional inf-norms of the resulting rows and columns accumulated into rown[i] / coln[j] by atomic max.
//   SYM: only the upper triangle i <= j is stored / touched and both norms describe the symmetric matrix (rown == coln array); the products
//   are (M * scol) * srow (dense scale_P, preconditioner.hpp:119-124), otherwise (srow * M) * scol (A, G: :127-131).
template <bool SYM, bool VEC, bool NORMS, bool USE_PRE>
__global__ __launch_bounds__(TR) void k_rzd_pass(int rows, int cols, double* __restrict__ M, const double* __restrict__ srow, const double* __restrict__ scol, const double* pre_ptr,
                                                 double* rown, double* coln, const DenseState* st, int ignore_done)
{
    __shared__ double colmax[TC];
    if (!ignore_done && st->done) return;
    const int rb = blockIdx.x, cb = blockIdx.y;
    const int j0 = cb * TC, i = rb * TR + threadIdx.x;
    if (SYM && rb * TR > j0 + TC - 1) return;  // tile strictly below the diagonal
    const int jn = min(TC, cols - j0);
    if (NORMS) { if (threadIdx.x < TC) colmax[threadIdx.x] = 0.0; __syncthreads(); }
    const double pre = USE_PRE ? *pre_ptr : 1.0;
    const double si = (VEC && i < rows) ? srow[i] : 1.0;
    double rmax = 0.0;
    for (int jj = 0; jj < jn; ++jj) {
        const int j = j0 + jj;
        double a = 0.0;
        if (i < rows && (!SYM || i <= j)) {
            double* e = M + (size_t)j * rows + i;
            double v = *e;
            if (USE_PRE) v *= pre;
            if (VEC) v = SYM ? (v * scol[j]) * si : (si * v) * scol[j];
            if (VEC || USE_PRE) *e = v;
            a = fabs(v);
        }
        if (NORMS) {
            rmax = fmax(rmax, a);
            const double cm = wave_max(a);
            if ((threadIdx.x & 63) == 0) amax_lds(&colmax[jj], cm);
        }
    }
    if (NORMS) {
        if (i < rows) amax(rown + i, rmax);
        __syncthreads();
        if (threadIdx.x < jn) amax(coln + j0 + threadIdx.x, colmax[threadIdx.x]);
    }
}
// dense/preconditioner.hpp:112-117,133-139: this pass's scaling from the norms; c, x_b_scaling, delta, delta_b follow
__global__ void k_rzd_delta(int N, int n, double* di, double* dib, double* c, double* xbs, double* delta, double* delta_b, const DenseState* st)
{
    if (st->done) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (i < n) {
        const double xb = xbs[i];
        const double d = inv_sqrt_limited(fmax(di[i], xb)), db = inv_sqrt_limited(xb);
        di[i] = d; dib[i] = db;
        c[i] *= d;
        xbs[i] = xb * (db * d);
        delta_b[i] *= db;
        delta[i] *= d;
    } else {
        const double d = inv_sqrt_limited(di[i]);
        di[i] = d;
        delta[i] *= d;
    }
}
// :141-158 cost scaling: gamma = 1 / limit(max(limit(mean column norm of P), |c|_inf))
__global__ void k_rzd_gamma(int n, const double* tmp, double* c, DenseState* st)
{
    __shared__ double red[16];
    __shared__ double gsum;
    if (st->done) return;
    if (threadIdx.x == 0) {
        double g = 0.0;
        for (int k = 0; k < n; ++k) g += tmp[k];
        gsum = g;
    }
    double cinf = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) cinf = fmax(cinf, fabs(c[i]));
    cinf = block_max(cinf, red);
    double gamma = gsum / (double)n;
    gamma = limit_scaling(gamma);
    gamma = limit_scaling(fmax(gamma, cinf));
    gamma = 1.0 / gamma;
    for (int i = threadIdx.x; i < n; i += blockDim.x) c[i] *= gamma;
    if (threadIdx.x == 0) { st->gamma = gamma; st->c *= gamma; }
}
__global__ void k_rzd_finish(int N, int n, const double* delta, const double* delta_b, double* di, double* dib, DenseState* st)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) di[i] = 1.0 / delta[i];
    if (i < n) dib[i] = 1.0 / delta_b[i];
    if (i == 0) st->c_inv = 1.0 / st->c;
}
// the vector part of the reuse / unscale branches: c *= cs * s, x_b_scaling *= sb * s
__global__ void k_rzd_vectors(int n, double* c, double* xbs, const double* s, const double* sb, const double* cs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { c[i] *= *cs * s[i]; xbs[i] *= sb[i] * s[i]; }
}

thread_local RuizLaunch g_last_launch;  // what the test hook reports; written on the host beside each launch, read by nothing else

}  // namespace

RuizLaunch ruiz_last_launch() { return g_last_launch; }

void launch_ruiz_sparse(const RuizSparseArgs& a, int batch, int threads, hipStream_t s)
{
    if (batch <= 0) return;
    static const bool one_wg = debug_token("ruiz_one_wg") != nullptr;  // debugging aid: PIQP_AMD_DEBUG=ruiz_one_wg
    if (batch == 1 && a.grid_ws && a.max_iter <= 64 && !one_wg) {
        // one instance on the whole chip: workgroups of 256 threads, at most one per CU (every workgroup must be resident: grid barriers)
        int cus = 0, dev = 0;
        PQ_HIP(hipGetDevice(&dev));
        PQ_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const int N = a.n + a.p + a.m;
        // 512 rows per workgroup, at most 48 workgroups: a barrier costs more the more workgroups poll its counter (C3 pattern, N = 100 000: 5.3 ms on 49
        // workgroups, 12.4 ms on 196), and below 2048 rows four workgroups still halve the one-workgroup time (chain-mass N = 1822: update 1.9 -> 1.1 ms)
        const int g = std::max(1, std::min(std::min(cus > 0 ? cus : 64, 48), (N + 511) / 512));
        if (g > 1) {
            PQ_HIP(hipMemsetAsync(a.grid_ws, 0, sizeof(unsigned long long) * RUIZ_WS_WORDS, s));
            hipLaunchKernelGGL(k_ruiz_sparse<true>, dim3(g), dim3(256), 0, s, a);
            PQ_HIP(hipGetLastError());
            g_last_launch = RuizLaunch{PQ_RUIZ_LAUNCH_GRID, g, 1, 256};
            return;
        }
    }
    hipLaunchKernelGGL(k_ruiz_sparse<false>, dim3(batch), dim3(threads), 0, s, a);
    PQ_HIP(hipGetLastError());
    g_last_launch = RuizLaunch{PQ_RUIZ_LAUNCH_ONE_WG, batch, 1, threads};
}
size_t ruiz_grid_ws_words() { return RUIZ_WS_WORDS; }

// ------------------------------------------------------------------------------------------------ DeviceRuiz
struct DeviceRuiz::Impl {
    int device = 0, n = 0, p = 0, m = 0;
    bool sparse = false;
    // dense: the matrices (scaled once scale() ran); sparse: value staging
    DBuf<double> P, AT, GT;
    DBuf<int> Pp, Pi, ATp, ATi, GTp, GTi;
    DBuf<int> srcP, srcA, srcG, rows;  // sparse, device-fed: gather maps (stored position -> caller's CSC position), uploaded by the first ingest; disabled rows of G
    DBuf<double> vec;  // c | xbs | delta | delta_inv | delta_b | delta_b_inv | tmp
    DBuf<DenseState> state;
    DBuf<double> cscale;
    DBuf<unsigned long long> gridws;  // sparse: barrier counter and reduction slots of the grid-wide equilibration
    HBuf<double> hvec;
    double *c = nullptr, *xbs = nullptr, *delta = nullptr, *delta_inv = nullptr, *delta_b = nullptr, *delta_b_inv = nullptr, *tmp = nullptr;
    size_t vec_len = 0;
    Stream st;
};

DeviceRuiz::DeviceRuiz(int device, const HostData& d) : I(new Impl)
{
    Impl& s = *I;
    s.device = device; s.n = d.n; s.p = d.p; s.m = d.m; s.sparse = d.sparse;
    s.st = Stream(device);
    const size_t n = d.n, N = (size_t)d.n + d.p + d.m;
    s.vec_len = 5 * n + 2 * N;
    s.vec.alloc(s.vec_len);
    s.hvec.alloc(s.vec_len);
    double* v = s.vec.p;
    s.c = v; v += n; s.xbs = v; v += n; s.delta = v; v += N; s.delta_inv = v; v += N; s.delta_b = v; v += n; s.delta_b_inv = v; v += n; s.tmp = v;
    s.state.alloc(1);
    s.cscale.alloc(1);
    if (!d.sparse) {
        s.P.alloc(n * n);
        s.AT.alloc(n * (size_t)d.p);
        s.GT.alloc(n * (size_t)d.m);
    } else {
        auto up = [&](DBuf<int>& dst, const IVec& h) { dst.alloc(std::max<size_t>(h.size(), 1)); if (!h.empty()) PQ_HIP(hipMemcpyAsync(dst.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, s.st)); };
        up(s.Pp, d.sP_utri.colptr); up(s.Pi, d.sP_utri.rowind);
        up(s.ATp, d.sAT.colptr); up(s.ATi, d.sAT.rowind);
        up(s.GTp, d.sGT.colptr); up(s.GTi, d.sGT.rowind);
        s.P.alloc(std::max<size_t>(d.sP_utri.rowind.size(), 1));
        s.AT.alloc(std::max<size_t>(d.sAT.rowind.size(), 1));
        s.GT.alloc(std::max<size_t>(d.sGT.rowind.size(), 1));
        stream_wait(s.st);
    }
}
DeviceRuiz::~DeviceRuiz() = default;

std::unique_ptr<DeviceRuiz> DeviceRuiz::clone() const
{
    const Impl& s = *I;
    HostData shape;
    shape.sparse = false; shape.n = s.n; shape.p = s.p; shape.m = s.m;
    if (s.sparse) throw std::runtime_error("DeviceRuiz::clone: sparse instances are rebuilt from the host data");
    std::unique_ptr<DeviceRuiz> r(new DeviceRuiz(s.device, shape));
    Impl& t = *r->I;
    PQ_HIP(hipSetDevice(s.device));
    stream_wait(s.st);
    auto cp = [&](DBuf<double>& dst, const DBuf<double>& src) { if (src.n) PQ_HIP(hipMemcpyAsync(dst.p, src.p, src.bytes(), hipMemcpyDeviceToDevice, t.st)); };
    cp(t.P, s.P); cp(t.AT, s.AT); cp(t.GT, s.GT); cp(t.vec, s.vec);
    PQ_HIP(hipMemcpyAsync(t.state.p, s.state.p, sizeof(DenseState), hipMemcpyDeviceToDevice, t.st));
    stream_wait(t.st);
    return r;
}

void DeviceRuiz::upload_dense(const HostData& d, int options)
{
    Impl& s = *I;
    if (s.sparse) throw std::runtime_error("DeviceRuiz::upload_dense on a sparse problem");
    PQ_HIP(hipSetDevice(s.device));
    const size_t n = s.n;
    if ((options & PQ_KKT_UPDATE_P) && s.P.n) PQ_HIP(hipMemcpyAsync(s.P.p, d.P_utri.data(), s.P.bytes(), hipMemcpyHostToDevice, s.st));
    if ((options & PQ_KKT_UPDATE_A) && s.AT.n) PQ_HIP(hipMemcpyAsync(s.AT.p, d.AT.data(), n * s.p * sizeof(double), hipMemcpyHostToDevice, s.st));
    if ((options & PQ_KKT_UPDATE_G) && s.GT.n) PQ_HIP(hipMemcpyAsync(s.GT.p, d.GT.data(), n * s.m * sizeof(double), hipMemcpyHostToDevice, s.st));
    stream_wait(s.st);
}

long long DeviceRuiz::ingest_dense(const double* P, const double* A, const double* G, int layout, int options)
{
    Impl& s = *I;
    if (s.sparse) throw std::runtime_error("DeviceRuiz::ingest_dense on a sparse problem");
    PQ_HIP(hipSetDevice(s.device));
    const int n = s.n;
    long long moved = 0;
    if ((options & PQ_KKT_UPDATE_P) && P && s.P.n) {
        if (layout == PQ_ROW_MAJOR) ingest_transpose(s.P.p, P, n, n, true, s.st);  // a row-major P is the column-major P^T
        else ingest_copy_upper(s.P.p, P, n, s.st);
        moved += (long long)s.P.bytes();
    }
    auto mat = [&](DBuf<double>& dst, const double* src, int rows) {  // src rows x n -> dst = src^T, column-major n x rows
        if (!src || !dst.n) return;
        if (layout == PQ_ROW_MAJOR) PQ_HIP(hipMemcpyAsync(dst.p, src, dst.bytes(), hipMemcpyDeviceToDevice, s.st));
        else ingest_transpose(dst.p, src, rows, n, false, s.st);
        moved += (long long)dst.bytes();
    };
    if (options & PQ_KKT_UPDATE_A) mat(s.AT, A, s.p);
    if (options & PQ_KKT_UPDATE_G) mat(s.GT, G, s.m);
    stream_wait(s.st);
    return moved;
}

void DeviceRuiz::zero_G_rows(const std::vector<int>& rows)
{
    Impl& s = *I;
    if (rows.empty()) return;
    PQ_HIP(hipSetDevice(s.device));
    if (s.sparse) {
        if ((int)rows.size() > s.m) throw std::runtime_error("DeviceRuiz::zero_G_rows: more rows than G has");
        if (!s.rows.p) s.rows.alloc(std::max(s.m, 1));
        PQ_HIP(hipMemcpyAsync(s.rows.p, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, s.st));
        ingest_zero_columns(s.GT.p, s.GTp.p, s.rows.p, (int)rows.size(), s.st);
        stream_wait(s.st);  // (`rows` is the caller's)
        return;
    }
    for (int r : rows) PQ_HIP(hipMemsetAsync(s.GT.p + (size_t)r * s.n, 0, sizeof(double) * s.n, s.st));
    stream_wait(s.st);
}

long long DeviceRuiz::ingest_sparse(const HostData& d, const double* Px, const double* Ax, const double* Gx, int options)
{
    Impl& s = *I;
    if (!s.sparse) throw std::runtime_error("DeviceRuiz::ingest_sparse on a dense problem");
    PQ_HIP(hipSetDevice(s.device));
    const size_t nzP = d.sP_utri.rowind.size(), nzA = d.sAT.rowind.size(), nzG = d.sGT.rowind.size();
    if (d.srcP.size() != nzP || d.srcA.size() != nzA || d.srcG.size() != nzG) throw std::runtime_error("DeviceRuiz::ingest_sparse: no gather maps");
    if (std::max(nzP, std::max(nzA, nzG)) > (size_t)INT_MAX) throw std::runtime_error("DeviceRuiz::ingest_sparse: more than 2^31 - 1 nonzeros");  // (int32 CSC: cannot happen)
    if (!s.srcP.p) {
        auto up = [&](DBuf<int>& dst, const IVec& h) { dst.alloc(std::max<size_t>(h.size(), 1)); if (!h.empty()) PQ_HIP(hipMemcpyAsync(dst.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, s.st)); };
        up(s.srcP, d.srcP); up(s.srcA, d.srcA); up(s.srcG, d.srcG);
    }
    long long moved = 0;
    auto mat = [&](DBuf<double>& dst, const double* src, const DBuf<int>& map, size_t cnt) {
        if (!src || !cnt) return;
        ingest_gather(dst.p, src, map.p, (int)cnt, s.st);
        moved += (long long)(cnt * sizeof(double));
    };
    if (options & PQ_KKT_UPDATE_P) mat(s.P, Px, s.srcP, nzP);
    if (options & PQ_KKT_UPDATE_A) mat(s.AT, Ax, s.srcA, nzA);
    if (options & PQ_KKT_UPDATE_G) mat(s.GT, Gx, s.srcG, nzG);
    stream_wait(s.st);
    return moved;
}

void DeviceRuiz::copy_values_from(const DeviceRuiz& o)
{
    Impl& s = *I;
    const Impl& t = *o.I;
    if (!s.sparse || !t.sparse || s.P.n != t.P.n || s.AT.n != t.AT.n || s.GT.n != t.GT.n) throw std::runtime_error("DeviceRuiz::copy_values_from: not the same sparse problem");
    PQ_HIP(hipSetDevice(s.device));
    stream_wait(t.st);
    auto cp = [&](DBuf<double>& dst, const DBuf<double>& src) { PQ_HIP(hipMemcpyAsync(dst.p, src.p, src.bytes(), hipMemcpyDeviceToDevice, s.st)); };
    cp(s.P, t.P); cp(s.AT, t.AT); cp(s.GT, t.GT); cp(s.vec, t.vec);
    stream_wait(s.st);
}

// x_b_scaling: the device copy the last scale / unscale left, which is HostData::x_b_scaling bit for bit -- only those two change it, on the device, and download
// it (an update of vectors alone rescales c and the bounds, never x_b_scaling)
pq_sparse_data DeviceRuiz::sparse_descriptor(const HostData& d) const
{
    pq_sparse_data desc = d.sparse_descriptor();
    desc.P_val = I->P.p; desc.AT_val = I->AT.p; desc.GT_val = I->GT.p;
    desc.x_b_scaling = I->xbs;
    desc.mem = PQ_MEM_DEVICE;
    return desc;
}

pq_dense_data DeviceRuiz::dense_descriptor(const HostData& d) const
{
    pq_dense_data desc = d.dense_descriptor();
    desc.P_utri = I->P.p; desc.AT = I->AT.p; desc.GT = I->GT.p;
    desc.mem = PQ_MEM_DEVICE;
    return desc;
}

void DeviceRuiz::scale(HostData& d, Ruiz& rz, bool reuse_prev_scaling, bool scale_cost, int max_iter, double eps)
{
    run(d, rz, reuse_prev_scaling ? RUIZ_REUSE : RUIZ_COMPUTE, scale_cost, max_iter, eps);
}
void DeviceRuiz::unscale(HostData& d, Ruiz& rz) { run(d, rz, RUIZ_UNSCALE, false, 0, 0.0); }

void DeviceRuiz::run(HostData& d, Ruiz& rz, int mode, bool scale_cost, int max_iter, double eps)
{
    Impl& s = *I;
    PQ_HIP(hipSetDevice(s.device));
    const int n = s.n, p = s.p, m = s.m, N = n + p + m;
    hipStream_t st = s.st;
    // ---- host -> device: c, x_b_scaling (always), the scalings (reuse / unscale), the sparse values
    double* h = s.hvec.p;
    const size_t oc = 0, ox = n, od = 2 * (size_t)n, odi = od + N, odb = odi + N, odbi = odb + n;
    std::copy(d.c.begin(), d.c.begin() + n, h + oc);
    std::copy(d.x_b_scaling.begin(), d.x_b_scaling.begin() + n, h + ox);
    if (mode != RUIZ_COMPUTE) {
        std::copy(rz.delta.begin(), rz.delta.end(), h + od); std::copy(rz.delta_inv.begin(), rz.delta_inv.end(), h + odi);
        std::copy(rz.delta_b.begin(), rz.delta_b.end(), h + odb); std::copy(rz.delta_b_inv.begin(), rz.delta_b_inv.end(), h + odbi);
    }
    PQ_HIP(hipMemcpyAsync(s.vec.p, h, (odbi + n) * sizeof(double), hipMemcpyHostToDevice, st));
    if (s.sparse) {
        auto upv = [&](DBuf<double>& dst, const Vec& v) { if (!v.empty()) PQ_HIP(hipMemcpyAsync(dst.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, st)); };
        upv(s.P, d.sP_utri.val); upv(s.AT, d.sAT.val); upv(s.GT, d.sGT.val);
        PQ_HIP(hipMemcpyAsync(s.cscale.p, &rz.c, sizeof(double), hipMemcpyHostToDevice, st));
        RuizSparseArgs a;
        a.n = n; a.p = p; a.m = m;
        a.Pp = s.Pp.p; a.Pi = s.Pi.p; a.ATp = s.ATp.p; a.ATi = s.ATi.p; a.GTp = s.GTp.p; a.GTi = s.GTi.p;
        a.Px = s.P.p; a.ATx = s.AT.p; a.GTx = s.GT.p; a.c = s.c; a.xbs = s.xbs;
        a.delta = s.delta; a.delta_inv = s.delta_inv; a.delta_b = s.delta_b; a.delta_b_inv = s.delta_b_inv; a.tmp = s.tmp;
        a.c_scale = s.cscale.p;
        a.mode = mode; a.scale_cost = scale_cost; a.max_iter = max_iter; a.eps = eps;
        if (!s.gridws.p) s.gridws.alloc(ruiz_grid_ws_words());
        a.grid_ws = s.gridws.p;
        launch_ruiz_sparse(a, 1, 1024, st);
        auto dn = [&](Vec& v, const DBuf<double>& src) { if (!v.empty()) PQ_HIP(hipMemcpyAsync(v.data(), src.p, v.size() * sizeof(double), hipMemcpyDeviceToHost, st)); };
        dn(d.sP_utri.val, s.P); dn(d.sAT.val, s.AT); dn(d.sGT.val, s.GT);
        if (mode == RUIZ_COMPUTE) PQ_HIP(hipMemcpyAsync(&rz.c, s.cscale.p, sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
        DenseState* ds = s.state.p;
        const dim3 gP(div_up(n, TR), div_up(n, TC)), gA(div_up(n, TR), std::max(1, div_up(p, TC))), gG(div_up(n, TR), std::max(1, div_up(m, TC)));
        const int eb = 256, eg = div_up(N, eb);
        if (mode == RUIZ_COMPUTE) {
            hipLaunchKernelGGL(k_rzd_begin, dim3(eg), dim3(eb), 0, st, N, n, s.delta, s.delta_b, s.delta_inv, s.delta_b_inv, ds);
            for (int it = 0; it < max_iter; ++it) {
                hipLaunchKernelGGL(k_rzd_check, dim3(1), dim3(1024), 0, st, N, n, s.delta_inv, s.delta_b_inv, s.tmp, eps, ds);
                hipLaunchKernelGGL((k_rzd_pass<true, false, true, false>), gP, dim3(TR), 0, st, n, n, s.P.p, nullptr, nullptr, nullptr, s.delta_inv, s.delta_inv, ds, 0);
                if (p > 0) hipLaunchKernelGGL((k_rzd_pass<false, false, true, false>), gA, dim3(TR), 0, st, n, p, s.AT.p, nullptr, nullptr, nullptr, s.delta_inv, s.delta_inv + n, ds, 0);
                if (m > 0) hipLaunchKernelGGL((k_rzd_pass<false, false, true, false>), gG, dim3(TR), 0, st, n, m, s.GT.p, nullptr, nullptr, nullptr, s.delta_inv, s.delta_inv + n + p, ds, 0);
                hipLaunchKernelGGL(k_rzd_delta, dim3(eg), dim3(eb), 0, st, N, n, s.delta_inv, s.delta_b_inv, s.c, s.xbs, s.delta, s.delta_b, ds);
                if (scale_cost) hipLaunchKernelGGL((k_rzd_pass<true, true, true, false>), gP, dim3(TR), 0, st, n, n, s.P.p, s.delta_inv, s.delta_inv, nullptr, s.tmp, s.tmp, ds, 0);
                else hipLaunchKernelGGL((k_rzd_pass<true, true, false, false>), gP, dim3(TR), 0, st, n, n, s.P.p, s.delta_inv, s.delta_inv, nullptr, nullptr, nullptr, ds, 0);
                if (p > 0) hipLaunchKernelGGL((k_rzd_pass<false, true, false, false>), gA, dim3(TR), 0, st, n, p, s.AT.p, s.delta_inv, s.delta_inv + n, nullptr, nullptr, nullptr, ds, 0);
                if (m > 0) hipLaunchKernelGGL((k_rzd_pass<false, true, false, false>), gG, dim3(TR), 0, st, n, m, s.GT.p, s.delta_inv, s.delta_inv + n + p, nullptr, nullptr, nullptr, ds, 0);
                if (scale_cost) {
                    hipLaunchKernelGGL(k_rzd_gamma, dim3(1), dim3(1024), 0, st, n, s.tmp, s.c, ds);
                    hipLaunchKernelGGL((k_rzd_pass<true, false, false, true>), gP, dim3(TR), 0, st, n, n, s.P.p, nullptr, nullptr, &ds->gamma, nullptr, nullptr, ds, 0);
                }
            }
            hipLaunchKernelGGL(k_rzd_finish, dim3(eg), dim3(eb), 0, st, N, n, s.delta, s.delta_b, s.delta_inv, s.delta_b_inv, ds);
        } else {
            DenseState hs{rz.c, rz.c_inv, 1.0, 0};
            PQ_HIP(hipMemcpyAsync(ds, &hs, sizeof(DenseState), hipMemcpyHostToDevice, st));
            stream_wait(st);  // hs is a stack object
            const double *sv = mode == RUIZ_REUSE ? s.delta : s.delta_inv, *sb = mode == RUIZ_REUSE ? s.delta_b : s.delta_b_inv;
            const double* cs = mode == RUIZ_REUSE ? &ds->c : &ds->c_inv;
            hipLaunchKernelGGL((k_rzd_pass<true, true, false, true>), gP, dim3(TR), 0, st, n, n, s.P.p, sv, sv, cs, nullptr, nullptr, ds, 1);
            if (p > 0) hipLaunchKernelGGL((k_rzd_pass<false, true, false, false>), gA, dim3(TR), 0, st, n, p, s.AT.p, sv, sv + n, nullptr, nullptr, nullptr, ds, 1);
            if (m > 0) hipLaunchKernelGGL((k_rzd_pass<false, true, false, false>), gG, dim3(TR), 0, st, n, m, s.GT.p, sv, sv + n + p, nullptr, nullptr, nullptr, ds, 1);
            hipLaunchKernelGGL(k_rzd_vectors, dim3(div_up(n, eb)), dim3(eb), 0, st, n, s.c, s.xbs, sv, sb, cs);
        }
        PQ_HIP(hipGetLastError());
        g_last_launch = RuizLaunch{PQ_RUIZ_LAUNCH_DENSE, (int)gP.x, (int)gP.y, TR};
    }
    // ---- device -> host: c, x_b_scaling and (after a fresh equilibration) the scalings
    PQ_HIP(hipMemcpyAsync(h, s.vec.p, (odbi + n) * sizeof(double), hipMemcpyDeviceToHost, st));
    DenseState hs{};
    if (!s.sparse && mode == RUIZ_COMPUTE) PQ_HIP(hipMemcpyAsync(&hs, s.state.p, sizeof(DenseState), hipMemcpyDeviceToHost, st));
    stream_wait(st);
    std::copy(h + oc, h + oc + n, d.c.begin());
    std::copy(h + ox, h + ox + n, d.x_b_scaling.begin());
    if (mode == RUIZ_COMPUTE) {
        std::copy(h + od, h + od + N, rz.delta.begin()); std::copy(h + odi, h + odi + N, rz.delta_inv.begin());
        std::copy(h + odb, h + odb + n, rz.delta_b.begin()); std::copy(h + odbi, h + odbi + n, rz.delta_b_inv.begin());
        if (!s.sparse) rz.c = hs.c;
        rz.c_inv = 1.0 / rz.c;
    }
}

// ------------------------------------------------------------------------------------------------ test hook (pq_debug_ruiz)
namespace {
void check_csc(const char* nm, int rows, int cols, const int* cp, const int* ri, const double* v, bool upper)
{
    const std::string w = std::string("debug_ruiz: ") + nm;
    if (cols == 0) return;
    if (!cp || cp[0] != 0) throw std::runtime_error(w + ": bad colptr");
    for (int j = 0; j < cols; ++j) if (cp[j + 1] < cp[j]) throw std::runtime_error(w + ": colptr decreases");
    if (cp[cols] > 0 && (!ri || !v)) throw std::runtime_error(w + ": null arrays");
    for (int j = 0; j < cols; ++j)
        for (int q = cp[j]; q < cp[j + 1]; ++q)
            if (ri[q] < 0 || ri[q] >= rows || (upper && ri[q] > j)) throw std::runtime_error(w + (upper && ri[q] > j ? ": not upper triangular" : ": row index out of range"));
}
double ruiz_sentinel()
{
    const unsigned long long b = PQ_RUIZ_SENTINEL_BITS;
    double d;
    std::memcpy(&d, &b, sizeof d);
    return d;
}
}  // namespace

void debug_ruiz(pq_ruiz_io* io, int device)
{
    const int n = io->n, p = io->p, m = io->m, mode = io->mode;
    if (n < 1 || p < 0 || m < 0 || (long long)n + p + m > (1 << 22)) throw std::runtime_error("debug_ruiz: bad dimensions");
    if (mode < RUIZ_COMPUTE || mode > RUIZ_UNSCALE || io->max_iter < 0 || io->max_iter > 1000) throw std::runtime_error("debug_ruiz: bad mode or max_iter");
    if (io->path < PQ_RUIZ_SOLVER_DENSE || io->path > PQ_RUIZ_KERNEL) throw std::runtime_error("debug_ruiz: unknown path");
    const size_t N = (size_t)n + p + m;
    const bool sparse = io->path != PQ_RUIZ_SOLVER_DENSE, kernel = io->path == PQ_RUIZ_KERNEL;
    const int batch = kernel ? io->batch : 1;
    if (batch < 1 || batch > 1024) throw std::runtime_error("debug_ruiz: bad batch");
    if (!io->c || !io->x_b_scaling || !io->delta || !io->delta_inv || !io->delta_b || !io->delta_b_inv || !io->c_scale) throw std::runtime_error("debug_ruiz: null vector");
    size_t nz[3] = {(size_t)n * n, (size_t)n * p, (size_t)n * m};
    if (sparse) {
        if (!io->P_colptr) throw std::runtime_error("debug_ruiz: P: bad colptr");
        nz[0] = io->P_colptr[n]; nz[1] = p ? io->AT_colptr ? io->AT_colptr[p] : 0 : 0; nz[2] = m ? io->GT_colptr ? io->GT_colptr[m] : 0 : 0;
        check_csc("P", n, n, io->P_colptr, io->P_rowind, io->P, true);
        check_csc("AT", n, p, io->AT_colptr, io->AT_rowind, io->AT, false);
        check_csc("GT", n, m, io->GT_colptr, io->GT_rowind, io->GT, false);
    } else if (n > 8192 || !io->P || (p && !io->AT) || (m && !io->GT)) {
        throw std::runtime_error("debug_ruiz: dense: null matrix or n > 8192");
    }
    io->guards_len = 0;
    PQ_HIP(hipSetDevice(device));

    if (!kernel) {
        // ---- what Solver::setup / update do
        HostData d;
        d.sparse = sparse; d.n = n; d.p = p; d.m = m;
        auto csc = [&](Csc& M, int cols, const int* cp, const int* ri, const double* v, size_t cnt) {
            M.rows = n; M.cols = cols;
            if (cols) M.colptr.assign(cp, cp + cols + 1); else M.colptr.assign(1, 0);
            if (cnt) { M.rowind.assign(ri, ri + cnt); M.val.assign(v, v + cnt); }
        };
        if (sparse) {
            csc(d.sP_utri, n, io->P_colptr, io->P_rowind, io->P, nz[0]);
            csc(d.sAT, p, io->AT_colptr, io->AT_rowind, io->AT, nz[1]);
            csc(d.sGT, m, io->GT_colptr, io->GT_rowind, io->GT, nz[2]);
        } else {
            d.P_utri.assign(io->P, io->P + nz[0]);
            if (nz[1]) d.AT.assign(io->AT, io->AT + nz[1]);
            if (nz[2]) d.GT.assign(io->GT, io->GT + nz[2]);
        }
        d.c.assign(io->c, io->c + n);
        d.x_b_scaling.assign(io->x_b_scaling, io->x_b_scaling + n);
        Ruiz rz;
        rz.init(d);
        if (mode != RUIZ_COMPUTE) {
            rz.delta.assign(io->delta, io->delta + N); rz.delta_inv.assign(io->delta_inv, io->delta_inv + N);
            rz.delta_b.assign(io->delta_b, io->delta_b + n); rz.delta_b_inv.assign(io->delta_b_inv, io->delta_b_inv + n);
            rz.c = io->c_scale[0]; rz.c_inv = 1.0 / rz.c;
        }
        DeviceRuiz dr(device, d);
        if (!sparse) dr.upload_dense(d, PQ_KKT_UPDATE_P | PQ_KKT_UPDATE_A | PQ_KKT_UPDATE_G);
        g_last_launch = RuizLaunch{};
        if (mode == RUIZ_UNSCALE) dr.unscale(d, rz);
        else dr.scale(d, rz, mode == RUIZ_REUSE, io->scale_cost != 0, io->max_iter);
        if (sparse) {
            std::copy(d.sP_utri.val.begin(), d.sP_utri.val.end(), io->P);
            std::copy(d.sAT.val.begin(), d.sAT.val.end(), io->AT);
            std::copy(d.sGT.val.begin(), d.sGT.val.end(), io->GT);
        } else {
            const pq_dense_data desc = dr.dense_descriptor(d);
            PQ_HIP(hipMemcpy(io->P, desc.P_utri, nz[0] * sizeof(double), hipMemcpyDeviceToHost));
            if (nz[1]) PQ_HIP(hipMemcpy(io->AT, desc.AT, nz[1] * sizeof(double), hipMemcpyDeviceToHost));
            if (nz[2]) PQ_HIP(hipMemcpy(io->GT, desc.GT, nz[2] * sizeof(double), hipMemcpyDeviceToHost));
        }
        std::copy(d.c.begin(), d.c.end(), io->c);
        std::copy(d.x_b_scaling.begin(), d.x_b_scaling.end(), io->x_b_scaling);
        std::copy(rz.delta.begin(), rz.delta.end(), io->delta); std::copy(rz.delta_inv.begin(), rz.delta_inv.end(), io->delta_inv);
        std::copy(rz.delta_b.begin(), rz.delta_b.end(), io->delta_b); std::copy(rz.delta_b_inv.begin(), rz.delta_b_inv.end(), io->delta_b_inv);
        io->c_scale[0] = rz.c;
    } else {
        // ---- what the batched solver does: launch_ruiz_sparse on a strided arena, no grid workspace
        const int G = PQ_RUIZ_GUARD;
        if (io->threads < 64 || io->threads > 1024 || io->threads % 64) throw std::runtime_error("debug_ruiz: threads must be a multiple of 64 up to 1024");
        const int nxl = io->n_x_l, nxu = io->n_x_u;
        if (nxl < 0 || nxl > n || nxu < 0 || nxu > n || (io->x_l && nxl && !io->x_l_idx) || (io->x_u && nxu && !io->x_u_idx)) throw std::runtime_error("debug_ruiz: bad box index lists");
        for (int k = 0; io->x_l && k < nxl; ++k) if (io->x_l_idx[k] < 0 || io->x_l_idx[k] >= n) throw std::runtime_error("debug_ruiz: x_l_idx out of range");
        for (int k = 0; io->x_u && k < nxu; ++k) if (io->x_u_idx[k] < 0 || io->x_u_idx[k] >= n) throw std::runtime_error("debug_ruiz: x_u_idx out of range");
        enum { F_PX, F_ATX, F_GTX, F_C, F_XBS, F_DL, F_DLI, F_DB, F_DBI, F_TMP, F_B, F_HL, F_HU, F_XL, F_XU, F_COUNT };
        const size_t len[F_COUNT] = {nz[0], nz[1], nz[2], (size_t)n, (size_t)n, N, N, (size_t)n, (size_t)n, (size_t)n, (size_t)p, (size_t)m, (size_t)m, (size_t)nxl, (size_t)nxu};
        double* host[F_COUNT] = {io->P, io->AT, io->GT, io->c, io->x_b_scaling, io->delta, io->delta_inv, io->delta_b, io->delta_b_inv, nullptr, io->b, io->h_l, io->h_u, io->x_l, io->x_u};
        size_t off[F_COUNT], need = G;
        for (int f = 0; f < F_COUNT; ++f) { off[f] = need; need += len[f] + G; }
        if (io->stride < (long long)need || io->stride > (1LL << 26)) throw std::runtime_error("debug_ruiz: stride " + std::to_string(io->stride) + " does not hold the layout of " + std::to_string(need) + " doubles");
        const size_t stride = (size_t)io->stride, total = (size_t)batch * stride + G;
        const double S = ruiz_sentinel();
        std::vector<double> arena(total, S), cs((size_t)batch + 2 * G, S);
        std::vector<char> is_field(total, 0);
        const bool reads_scalings = mode != RUIZ_COMPUTE;
        for (int b = 0; b < batch; ++b)
            for (int f = 0; f < F_COUNT; ++f) {
                const bool present = f == F_TMP || host[f] != nullptr;
                if (!present || !len[f]) continue;
                double* dst = arena.data() + b * stride + off[f];
                std::fill(is_field.begin() + (b * stride + off[f]), is_field.begin() + (b * stride + off[f] + len[f]), 1);
                const bool scaling = f >= F_DL && f <= F_DBI;
                if (f != F_TMP && (!scaling || reads_scalings)) std::copy(host[f] + b * len[f], host[f] + (b + 1) * len[f], dst);
            }
        if (reads_scalings) std::copy(io->c_scale, io->c_scale + batch, cs.begin() + G);
        Stream st(device);
        DBuf<double> dArena(total), dCs(cs.size());
        DBuf<int> ip[8];
        auto upi = [&](DBuf<int>& dst, const int* h, size_t cnt) -> const int* {
            dst.alloc(std::max<size_t>(cnt, 1));
            if (cnt) PQ_HIP(hipMemcpyAsync(dst.p, h, cnt * sizeof(int), hipMemcpyHostToDevice, st));
            return dst.p;
        };
        RuizSparseArgs a;
        a.n = n; a.p = p; a.m = m;
        a.Pp = upi(ip[0], io->P_colptr, (size_t)n + 1); a.Pi = upi(ip[1], io->P_rowind, nz[0]);
        a.ATp = upi(ip[2], io->AT_colptr, p ? (size_t)p + 1 : 0); a.ATi = upi(ip[3], io->AT_rowind, nz[1]);
        a.GTp = upi(ip[4], io->GT_colptr, m ? (size_t)m + 1 : 0); a.GTi = upi(ip[5], io->GT_rowind, nz[2]);
        a.x_l_idx = upi(ip[6], io->x_l_idx, io->x_l ? (size_t)nxl : 0); a.x_u_idx = upi(ip[7], io->x_u_idx, io->x_u ? (size_t)nxu : 0);
        a.n_x_l = nxl; a.n_x_u = nxu;
        a.stride = io->stride;
        auto at = [&](int f) { return dArena.p + off[f]; };
        a.Px = at(F_PX); a.ATx = at(F_ATX); a.GTx = at(F_GTX); a.c = at(F_C); a.xbs = at(F_XBS);
        a.delta = at(F_DL); a.delta_inv = at(F_DLI); a.delta_b = at(F_DB); a.delta_b_inv = at(F_DBI); a.tmp = at(F_TMP);
        a.b = io->b ? at(F_B) : nullptr; a.h_l = io->h_l ? at(F_HL) : nullptr; a.h_u = io->h_u ? at(F_HU) : nullptr;
        a.x_l = io->x_l ? at(F_XL) : nullptr; a.x_u = io->x_u ? at(F_XU) : nullptr;
        a.c_scale = dCs.p + G;
        a.mode = mode; a.scale_cost = io->scale_cost != 0; a.max_iter = io->max_iter;
        PQ_HIP(hipMemcpyAsync(dArena.p, arena.data(), total * sizeof(double), hipMemcpyHostToDevice, st));
        PQ_HIP(hipMemcpyAsync(dCs.p, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice, st));
        g_last_launch = RuizLaunch{};
        launch_ruiz_sparse(a, batch, io->threads, st);
        PQ_HIP(hipMemcpyAsync(arena.data(), dArena.p, total * sizeof(double), hipMemcpyDeviceToHost, st));
        PQ_HIP(hipMemcpyAsync(cs.data(), dCs.p, cs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        stream_wait(st);
        for (int b = 0; b < batch; ++b)
            for (int f = 0; f < F_COUNT; ++f)
                if (f != F_TMP && host[f] && len[f]) std::copy(arena.data() + b * stride + off[f], arena.data() + b * stride + off[f] + len[f], host[f] + b * len[f]);
        std::copy(cs.begin() + G, cs.begin() + G + batch, io->c_scale);
        long long g = 0;
        auto guard = [&](double v) { if (io->guards && g < io->guards_cap) io->guards[g] = v; ++g; };
        for (size_t i = 0; i < total; ++i) if (!is_field[i]) guard(arena[i]);
        for (int i = 0; i < G; ++i) guard(cs[i]);
        for (int i = 0; i < G; ++i) guard(cs[(size_t)G + batch + i]);
        if (!io->guards || g > io->guards_cap) throw std::runtime_error("debug_ruiz: guards_cap too small: " + std::to_string(g) + " guard doubles");
        io->guards_len = g;
    }
    const RuizLaunch l = ruiz_last_launch();
    io->launch[0] = l.kernel; io->launch[1] = l.gx; io->launch[2] = l.gy; io->launch[3] = l.threads;
}

}  // namespace pq
