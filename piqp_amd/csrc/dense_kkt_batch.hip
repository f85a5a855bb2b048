// piqp_amd/csrc/dense_kkt_batch.hip -- pq_kkt_batch_*: piqp::dense::KKT (dense/kkt.hpp:39-160) for a BATCH of small QPs (n <= 128; p, m unlimited) that share
// n, p, m and the factorisation kind.  Per instance the assembled matrix, the factor, the success flag, every solve and the three mat-vec evaluators are those of
// the CPU oracle's dense backend (oracle/orc_dense.c as oracle/Makefile builds it: -ffp-contract=fast, so its multiply-adds are fused) bit for bit.  This file is
// compiled with -ffp-contract=off (piqp_amd/build.py, NO_CONTRACT): every fused operation below is an explicit fma(), everything else rounds on its own.  Each
// element is one sequential chain and elements are independent, so the parallelism is across elements (and across the batch); no matrix instruction is used.
//
//   oracle (orc_dense.c)                      here
//   dense_factor :643                         k_kb_factor: z_reg_inv[k] = 1.0 / z_reg[k] (stored; the assembly forms the same quotient again for the slice it stages)
//   dense_update_kkt :616-636                 kb_assemble, the prologue, per element (i, j), i >= j, of the LDS square:  v = P_utri[j + i n],  on the diagonal
//                                             v = v + x_reg[j],  with p > 0  v = fma(1.0 / delta, AT_A[i + j n], v)   (k_ex_syrk's prologue in dense_exact.hip)
//   syrk_like_lower (GT, z_reg_inv)           kb_assemble, per element and K block of 256 in ascending order:  acc = 0,  acc = fma(GT[i, k], 0.0 + z_reg_inv[k] * GT[j, k], acc)
//                                             for ascending k,  v = v + acc.  GT comes through LDS in slices of 16 columns (16 divides 256: a block boundary is a slice
//                                             boundary); between the slices of a block acc rests in the element's mirror place in the upper triangle of the square
//                                             (diagonal elements: in a vector of n beside it), v in the element's own place
//   dense_compute_ATA :593-598                k_kb_assemble with P_utri = null and no weights: v = 0.0, the same loop over AT, so the first block gives 0.0 + acc
//   orc_llt_compute /                         dfb_factor_in_lds (dense_factor_batch_device.hpp), the factorisation of dense_factor_batch.hip, on the square where the
//   orc_ldlt_no_pivot_compute                 assembly left it: the assembled matrix never goes to memory on the hot path
//   dense_solve :672-688                      k_kb_solve, one workgroup per instance, the factor in LDS.  Right-hand side (k_ex_rhs): thread i  c = rhs_x[i],
//                                             c = fma(GT[i, j], z_reg_inv[j] * rhs_z[j], c) for ascending j, then c = fma(AT[i, j], (1.0 / delta) * rhs_y[j], c)
//   orc_llt_solve_inplace /                   forward sweep column-oriented, thread i owns x_i:  (LLT x_j = x_j / l_jj,)  x_i = fma(-l_ij, x_j, x_i) for every i > j;
//   orc_ldlt_no_pivot_solve_inplace           LDLT then x_j = x_j / d_j;  backward sweep by ex_dot's rule (dense_exact.hip): s = x_j,  s = s - l_ij * x_i for ascending
//                                             i > j with the products rounded on their own, only the last of an odd count fused;  LLT x_j = s / l_jj.  The chain starts
//                                             at the value finished last, so the sweep is one dependent chain (thread 0 walks it, the others form the products of
//                                             the next column meanwhile -- k_ex_sweeps' scheme)
//   gemv_t + the two epilogues :684-687       one thread per output:  s = ex_dot(column j, lhs_x);  lhs_y[j] = fma(-dinv, rhs_y[j], dinv * s);
//                                             lhs_z[j] = ((1.0 * s) - rhs_z[j]) * z_reg_inv[j]   (k_ex_gemv_t modes 1 and 2)
//   dense_eval_P_x, dense_eval_A / _G         k_kb_eval_P, k_kb_eval_NT: one thread per output element and instance, k_ex_eval_P / k_ex_gemv_t mode 0 / k_ex_gemv_n
//
// Launch shape: the batched factor's.  n >= 32: one workgroup of 256 per instance; n < 32: four instances per workgroup, one wave each (the last workgroup of a
// batch that is no multiple of four runs partly empty).  The grid is the batch; a launch wider than the chip queues; no workgroup waits for another.
// LDS per instance: the square with leading dimension n | 1, n doubles for the diagonal's accumulators, a slice of 16 columns of GT and its 16 weights:
// n (n | 1) + 17 n + 16 doubles = 146.1 KiB at n = 128 of the compute unit's 160 KiB (one workgroup per compute unit there; several below).
// The per-instance pieces (kb_assemble, dfb_factor_in_lds, kb_rhs_row, kb_sweeps, kb_epilogues, the evaluators' kb_* functions) take pointers to ONE instance's
// data, so a kernel that iterates on an instance can call them as they are: they live in dense_kkt_batch_device.hpp, the handle in dense_kkt_batch_internal.hpp, and
// dense_kktsys_batch.hip (pq_kktsys_batch_*) is that kernel.
#include <chrono>
#include <cmath>
#include <memory>

#include "dense_kkt_batch_internal.hpp"

namespace pq {

namespace {

struct KbFactorArgs {
    int n, p, m, ld, width, batch;
    const double *Pu, *ATA, *GT;           // the handle's data: [batch][n n], [batch][n n] (null when p == 0), [batch][n m]
    const double *delta, *x_reg, *z_reg;   // this call's scalings: [batch], [batch][n], [batch][m]
    double *delta_s, *x_reg_s, *zinv_s;    // the handle's copies of them (z_reg as its reciprocal)
    double* F;                             // [batch][n n], leading dimension n, lower triangle written on success
    int *info, *badcol;                    // 0 / 1; -1 or the failing column
};

// update_scalings_and_factor of every instance: reciprocal, assembly into LDS, factorisation, the factor to memory
template <int KIND, int G>
__global__ __launch_bounds__(DFB_THREADS) void k_kb_factor(const KbFactorArgs A)
{
    extern __shared__ double kb_lds[];
    constexpr int MPW = DFB_THREADS / G;
    __shared__ int s_fail[MPW];
    const int n = A.n, m = A.m, ld = A.ld;
    const int g = threadIdx.x / G, t = threadIdx.x % G;
    const long long inst = (long long)blockIdx.x * MPW + g;
    const bool have = inst < A.batch;
    double* a = kb_lds + (size_t)g * ((size_t)n * ld + (size_t)(KB_SLICE + 1) * n + KB_SLICE);
    double* dacc = a + (size_t)n * ld;
    double* gs = dacc + n;
    double* ws = gs + (size_t)KB_SLICE * n;
    if (t == 0) s_fail[g] = -1;
    const size_t nn = (size_t)n * n;
    const double* x_reg = have ? A.x_reg + inst * n : nullptr;
    const double* z_reg = have ? A.z_reg + inst * m : nullptr;
    double dinv = 1.0;
    if (have) {
        const double delta = A.delta[inst];
        dinv = 1.0 / delta;
        if (t == 0) A.delta_s[inst] = delta;
        for (int i = t; i < n; i += G) A.x_reg_s[inst * n + i] = x_reg[i];
        for (int k = t; k < m; k += G) A.zinv_s[inst * m + k] = 1.0 / z_reg[k];
    }
    kb_assemble<G>(a, dacc, gs, ws, n, ld, m, have ? A.GT + inst * (size_t)n * m : nullptr, m > 0 ? z_reg : nullptr, true, have ? A.Pu + inst * nn : nullptr, x_reg,
                   have && A.ATA ? A.ATA + inst * nn : nullptr, dinv, have, t);
    const bool live = dfb_factor_in_lds<KIND, G>(a, n, ld, A.width, have, g, t, s_fail);
    if (!have) return;
    if (t == 0) { A.info[inst] = live ? 0 : 1; A.badcol[inst] = s_fail[g]; }
    if (!live) return;
    double* dst = A.F + inst * nn;
    for (int e = t; e < n * n; e += G) {
        const int j = e / n, i = e % n;
        if (i >= j) dst[e] = a[i + j * ld];
    }
}

// The assemble-only instantiation: the lower triangle of  init + M diag(w) M'  of every instance to memory (out: [batch][n n], leading dimension n).  AT_A at
// create / update_data (Pu = null, M = AT, no weights) and the test hook pq_kkt_batch_internal_kkt_mat (one instance, the stored scalings).  list: null = slot s of
// the grid is instance s; else `batch` counts the slots and slot s works on instance list[s] -- M, w, Pu, x_reg, ATA, delta and out are all reached by INSTANCE.
template <int G>
__global__ __launch_bounds__(DFB_THREADS) void k_kb_assemble(int n, int ld, int batch, int kdim, const double* __restrict__ M, const double* __restrict__ w,
                                                            const double* __restrict__ Pu, const double* __restrict__ x_reg, const double* __restrict__ ATA,
                                                            const double* __restrict__ delta, double* __restrict__ out, const int* __restrict__ list)
{
    extern __shared__ double kb_lds[];
    constexpr int MPW = DFB_THREADS / G;
    const int g = threadIdx.x / G, t = threadIdx.x % G;
    const long long slot = (long long)blockIdx.x * MPW + g;
    const bool have = slot < batch;
    const long long inst = list && have ? list[slot] : slot;
    double* a = kb_lds + (size_t)g * ((size_t)n * ld + (size_t)(KB_SLICE + 1) * n + KB_SLICE);
    double* dacc = a + (size_t)n * ld;
    double* gs = dacc + n;
    double* ws = gs + (size_t)KB_SLICE * n;
    const size_t nn = (size_t)n * n;
    const double dinv = have && delta ? 1.0 / delta[inst] : 1.0;
    kb_assemble<G>(a, dacc, gs, ws, n, ld, kdim, have ? M + inst * (size_t)n * kdim : nullptr, have && w ? w + inst * kdim : nullptr, false,
                   have && Pu ? Pu + inst * nn : nullptr, have && x_reg ? x_reg + inst * n : nullptr, have && ATA ? ATA + inst * nn : nullptr, dinv, have, t);
    if (!have) return;
    double* dst = out + inst * nn;
    for (int e = t; e < n * n; e += G) {
        const int j = e / n, i = e % n;
        if (i >= j) dst[e] = a[i + j * ld];
    }
}

// ---- solve (kb_rhs_row, kb_sweeps, kb_epilogues: dense_kkt_batch_device.hpp)
struct KbSolveArgs {
    int n, p, m, ld;
    const double *AT, *GT, *F, *delta_s, *zinv_s;
    const int* info;
    const double *rhs_x, *rhs_y, *rhs_z;
    double *lhs_x, *lhs_y, *lhs_z;
};

// dense_solve of every instance: blockIdx.x = instance.  An instance whose factorisation failed returns at once: its lhs blocks are not touched.
template <int KIND>
__global__ __launch_bounds__(KB_SOLVE_THREADS) void k_kb_solve(const KbSolveArgs A)
{
    extern __shared__ double kb_lds[];
    const long long inst = blockIdx.x;
    if (A.info[inst] != 0) return;  // (uniform: before any barrier)
    const int n = A.n, p = A.p, m = A.m, ld = A.ld, t = threadIdx.x;
    double* a = kb_lds;
    double* xs = a + (size_t)n * ld;
    double* pr = xs + n;
    double* xb = pr + 2 * (size_t)n;
    const double* src = A.F + inst * (size_t)n * n;
    for (int e = t; e < n * n; e += blockDim.x) {
        const int j = e / n, i = e % n;
        if (i >= j) a[i + j * ld] = src[e];
    }
    const double* GT = A.GT + inst * (size_t)n * m;
    const double* AT = A.AT + inst * (size_t)n * p;
    const double* zinv = A.zinv_s + inst * m;
    const double* rhs_y = A.rhs_y + inst * p;
    const double* rhs_z = A.rhs_z + inst * m;
    const double dinv = 1.0 / A.delta_s[inst];
    double c = 0.0;
    if (t < n) c = kb_rhs_row(t, n, p, m, GT, AT, zinv, dinv, A.rhs_x + inst * n, rhs_y, rhs_z);
    __syncthreads();
    kb_sweeps<KIND>(a, n, ld, c, xs, pr, xb, t);
    if (t < n) A.lhs_x[inst * n + t] = xs[t];
    kb_epilogues(n, p, m, GT, AT, zinv, dinv, xs, rhs_y, rhs_z, A.lhs_y + inst * p, A.lhs_z + inst * m, t, blockDim.x);
}

// ---- evaluators: one thread per output element and instance (blockIdx.y = instance)
__global__ __launch_bounds__(KB_EVAL_THREADS) void k_kb_eval_P(int n, const double* __restrict__ Pu, const double* __restrict__ alpha, const double* __restrict__ x,
                                                               double* __restrict__ z)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const long long inst = blockIdx.y;
    if (t >= n) return;
    z[inst * n + t] = kb_eval_P_row(t, n, Pu + inst * (size_t)n * n, alpha[inst], x + inst * n);
}

// eval_A_xn_and_AT_xt / eval_G_xn_and_GT_xt: M = AT resp. GT (n x cols).  Outputs o < cols: zn[o]; cols <= o < cols + n: zt[o - cols].
__global__ __launch_bounds__(KB_EVAL_THREADS) void k_kb_eval_NT(int n, int cols, const double* __restrict__ M, const double* __restrict__ alpha_n,
                                                                const double* __restrict__ alpha_t, const double* __restrict__ xn, const double* __restrict__ xt,
                                                                double* __restrict__ zn, double* __restrict__ zt)
{
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    const long long inst = blockIdx.y;
    const double* Mi = M + inst * (size_t)n * cols;
    if (o < cols) zn[inst * cols + o] = kb_gemv_t_col(o, n, Mi, xn + inst * n, alpha_n[inst]);
    else if (o < cols + n) zt[inst * n + (o - cols)] = kb_gemv_n_row(o - cols, n, cols, Mi, xt + inst * cols, alpha_t[inst]);
}

}  // namespace

}  // namespace pq

using namespace pq;

namespace {

void kb_raise_lds()
{
    // the square at n = 128 with its slice (146 KiB; the solve's 132 KiB) is more than the 64 KiB a launch may ask for by default
    static PerDeviceOnce once;
    once([&] {
        const int fb = (int)kb_factor_lds_bytes(PQ_KKT_BATCH_DENSE_MAX_N), sb = (int)kb_solve_lds_bytes(PQ_KKT_BATCH_DENSE_MAX_N);
        PQ_HIP(hipFuncSetAttribute((const void*)k_kb_factor<0, DFB_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, fb));
        PQ_HIP(hipFuncSetAttribute((const void*)k_kb_factor<1, DFB_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, fb));
        PQ_HIP(hipFuncSetAttribute((const void*)k_kb_assemble<DFB_THREADS>, hipFuncAttributeMaxDynamicSharedMemorySize, fb));
        PQ_HIP(hipFuncSetAttribute((const void*)k_kb_solve<0>, hipFuncAttributeMaxDynamicSharedMemorySize, sb));
        PQ_HIP(hipFuncSetAttribute((const void*)k_kb_solve<1>, hipFuncAttributeMaxDynamicSharedMemorySize, sb));
    });
}

void kb_alloc(pq_kkt_batch* k)
{
    const size_t b = (size_t)k->batch, n = (size_t)k->n, p = (size_t)k->p, m = (size_t)k->m, nn = n * n;
    k->st = Stream(k->device);
    k->Pu.alloc(b * nn); k->AT.alloc(b * n * p); k->GT.alloc(b * n * m);
    if (p > 0) k->ATA.alloc(b * nn);
    k->fac.alloc(b * nn); k->delta_s.alloc(b); k->x_reg_s.alloc(b * n); k->zinv_s.alloc(b * m); k->mat_d.alloc(nn);
    k->stage_in.alloc(b * (n + p + m + 2)); k->stage_out.alloc(b * (n + p + m));
    k->status.alloc(2 * b); k->status_h.alloc(2 * b); k->mat_h.alloc(nn);
    for (Event& e : k->ev) e = Event(0);
    k->fac.zero(k->st);  // the upper triangles stay zero for life
    k->mat_d.zero(k->st);
    kb_raise_lds();
}

// launches the assemble-only kernel over `count` instances with the factorisation's launch shape
void kb_launch_assemble(const pq_kkt_batch* k, int count, int kdim, const double* M, const double* w, const double* Pu, const double* x_reg, const double* ATA,
                        const double* delta, double* out, const int* list = nullptr)
{
    const int n = k->n, ld = dfb_ld(n);
    const size_t lds = kb_factor_lds_bytes(n);
    if (n < 32) k_kb_assemble<64><<<div_up(count, DFB_THREADS / 64), DFB_THREADS, lds, k->st>>>(n, ld, count, kdim, M, w, Pu, x_reg, ATA, delta, out, list);
    else k_kb_assemble<DFB_THREADS><<<count, DFB_THREADS, lds, k->st>>>(n, ld, count, kdim, M, w, Pu, x_reg, ATA, delta, out, list);
    PQ_HIP(hipGetLastError());
}

// dense/kkt.hpp:53: AT_A.lower = AT * AT^T of every instance, or of the `count` instances of a device list
void kb_compute_ata(pq_kkt_batch* k, const int* list = nullptr, int count = 0)
{
    if (k->p > 0) kb_launch_assemble(k, list ? count : k->batch, k->p, k->AT.p, nullptr, nullptr, nullptr, nullptr, nullptr, k->ATA.p, list);
}

}  // namespace

void pq::kb_refresh_ata(pq_kkt_batch* k, const int* list, int count) { kb_compute_ata(k, list, count); }

int pq::kb_factor_done(pq_kkt_batch* k, const std::chrono::steady_clock::time_point* w0, const KbReadback* more, int n_more)
{
    hipStream_t st = k->st;
    PQ_HIP(hipMemcpyAsync(k->status_h.p, k->status.p, sizeof(int) * 2 * k->batch, hipMemcpyDeviceToHost, st));
    for (int i = 0; i < n_more; ++i) PQ_HIP(hipMemcpyAsync(more[i].host, more[i].dev, more[i].bytes, hipMemcpyDeviceToHost, st));
    stream_wait(st);
    if (w0) {
        k->timed[0] = true;
        k->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - *w0).count();
    }
    int good = 0;
    for (int b = 0; b < k->batch; ++b) good += k->status_h.p[b] == 0;
    k->n_ok = good;
    k->computed = true;
    return good;
}

// instance j of the new handle is instance sel.host[j] of k: the data, A'A, the factor store, the stored scalings and both halves of the status ([0, batch): info,
// [batch, 2 batch): the first bad column -- two arrays in one buffer, one gather each) are gathered; the staging, mat_d and the events are only sized.  The new
// handle's stream is waited for before it is handed out, so the list at sel.dev may be released by the caller.
pq_kkt_batch* pq::kb_clone_rows(const pq_kkt_batch* k, const KbSelect& sel)
{
    PQ_HIP(hipSetDevice(k->device));
    stream_wait(k->st);
    std::unique_ptr<pq_kkt_batch> c(new pq_kkt_batch);
    c->device = k->device; c->batch = sel.count; c->n = k->n; c->p = k->p; c->m = k->m; c->kind = k->kind;
    kb_alloc(c.get());
    const size_t b = (size_t)sel.count, n = (size_t)k->n, nn = n * n;
    hipStream_t st = c->st;
    auto rows = [&](DBuf<double>& dst, const DBuf<double>& src, size_t len) { if (src.n) kb_gather_rows(st, dst.p, src.p, sel.dev, b, sizeof(double) * len); };
    PQ_HIP(hipEventRecord(c->ev[0], st));
    rows(c->Pu, k->Pu, nn); rows(c->AT, k->AT, n * k->p); rows(c->GT, k->GT, n * k->m); rows(c->ATA, k->ATA, nn); rows(c->fac, k->fac, nn);
    rows(c->delta_s, k->delta_s, 1); rows(c->x_reg_s, k->x_reg_s, n); rows(c->zinv_s, k->zinv_s, (size_t)k->m);
    for (int h = 0; h < 2; ++h) {
        kb_gather_rows(st, c->status.p + h * b, k->status.p + (size_t)h * k->batch, sel.dev, b, sizeof(int));
        kb_gather_host(c->status_h.p + h * b, k->status_h.p + (size_t)h * k->batch, sel.host, sel.count, 1);
    }
    c->computed = k->computed;
    for (int j = 0; j < sel.count && k->computed; ++j) c->n_ok += c->status_h.p[j] == 0;
    PQ_HIP(hipEventRecord(c->ev[1], st));
    kb_gather_timed(sel, st, c->ev[0], c->ev[1]);
    return c.release();
}

extern "C" {

int pq_kkt_batch_create_dense(pq_kkt_batch** out, int device, int batch, int n, int p, int m, int kkt_solver, const double* P_utri, const double* AT,
                              const double* GT, int mem)
{
    if (!out) return fail(PQ_ERR_INVALID, "null argument");
    if (batch < 1 || n < 1 || p < 0 || m < 0) return fail(PQ_ERR_INVALID, "dense KKT batch: batch = %d, n = %d, p = %d, m = %d: batch, n >= 1 and p, m >= 0 wanted", batch, n, p, m);
    if (kkt_solver != PQ_DENSE_CHOLESKY && kkt_solver != PQ_DENSE_LDLT_NO_PIVOT) return fail(PQ_ERR_INVALID, "dense KKT batch: kkt_solver %d is neither dense_cholesky nor dense_ldlt_no_pivot", kkt_solver);
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense KKT batch: bad mem");
    if (!P_utri || (p > 0 && !AT) || (m > 0 && !GT)) return fail(PQ_ERR_INVALID, "dense KKT batch: null matrix (P_utri, or AT with p > 0, or GT with m > 0)");
    if (n > PQ_KKT_BATCH_DENSE_MAX_N) return fail(PQ_ERR_UNSUPPORTED, "dense KKT batch: n = %d, the limit is n <= %d", n, (int)PQ_KKT_BATCH_DENSE_MAX_N);
    return guarded([&] {
        PQ_HIP(hipSetDevice(device));
        std::unique_ptr<pq_kkt_batch> k(new pq_kkt_batch);
        k->device = device; k->batch = batch; k->n = n; k->p = p; k->m = m; k->kind = kkt_solver;
        kb_alloc(k.get());
        copy_in(k->Pu.p, P_utri, k->Pu.bytes(), mem, k->st);
        copy_in(k->AT.p, AT, k->AT.bytes(), mem, k->st);
        copy_in(k->GT.p, GT, k->GT.bytes(), mem, k->st);
        kb_compute_ata(k.get());
        stream_wait(k->st);
        *out = k.release();
        return (int)PQ_OK;
    });
}

void pq_kkt_batch_destroy(pq_kkt_batch* k) { delete k; }

int pq_kkt_batch_clone(const pq_kkt_batch* k, pq_kkt_batch** out)
{
    if (!k || !out) return fail(PQ_ERR_INVALID, "null argument");
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        stream_wait(k->st);
        std::unique_ptr<pq_kkt_batch> c(new pq_kkt_batch);
        c->device = k->device; c->batch = k->batch; c->n = k->n; c->p = k->p; c->m = k->m; c->kind = k->kind;
        c->computed = k->computed; c->n_ok = k->n_ok;
        kb_alloc(c.get());
        auto cp = [&](DBuf<double>& dst, const DBuf<double>& src) { if (src.n) PQ_HIP(hipMemcpyAsync(dst.p, src.p, src.bytes(), hipMemcpyDeviceToDevice, c->st)); };
        cp(c->Pu, k->Pu); cp(c->AT, k->AT); cp(c->GT, k->GT); cp(c->ATA, k->ATA); cp(c->fac, k->fac); cp(c->delta_s, k->delta_s); cp(c->x_reg_s, k->x_reg_s); cp(c->zinv_s, k->zinv_s);
        PQ_HIP(hipMemcpyAsync(c->status.p, k->status.p, c->status.bytes(), hipMemcpyDeviceToDevice, c->st));
        std::memcpy(c->status_h.p, k->status_h.p, sizeof(int) * 2 * (size_t)k->batch);
        stream_wait(c->st);
        *out = c.release();
        return (int)PQ_OK;
    });
}

int pq_kkt_batch_clone_select(const pq_kkt_batch* k, const int* idx, int count, pq_kkt_batch** out)
{
    if (!k || !out) return fail(PQ_ERR_INVALID, "null argument");
    if (int rc = kb_check_select("dense KKT batch", k->batch, idx, count)) return rc;
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        DBuf<int> idx_d((size_t)count);
        PQ_HIP(hipMemcpy(idx_d.p, idx, sizeof(int) * (size_t)count, hipMemcpyHostToDevice));
        *out = kb_clone_rows(k, KbSelect{idx, idx_d.p, count, nullptr});
        return (int)PQ_OK;
    });
}

int pq_kkt_batch_dims(const pq_kkt_batch* k, int* batch, int* n, int* p, int* m)
{
    if (!k) return fail(PQ_ERR_INVALID, "null argument");
    if (batch) *batch = k->batch;
    if (n) *n = k->n;
    if (p) *p = k->p;
    if (m) *m = k->m;
    return PQ_OK;
}

int pq_kkt_batch_update_data_dense(pq_kkt_batch* k, const double* P_utri, const double* AT, const double* GT, int options, int mem)
{
    if (!k) return fail(PQ_ERR_INVALID, "null argument");
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense KKT batch: bad mem");
    if (((options & PQ_KKT_UPDATE_P) && !P_utri) || ((options & PQ_KKT_UPDATE_A) && !AT && k->p > 0) || ((options & PQ_KKT_UPDATE_G) && !GT && k->m > 0))
        return fail(PQ_ERR_INVALID, "dense KKT batch: update_data: a flagged matrix is null");
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        if (options & PQ_KKT_UPDATE_P) copy_in(k->Pu.p, P_utri, k->Pu.bytes(), mem, k->st);
        if (options & PQ_KKT_UPDATE_A) { copy_in(k->AT.p, AT, k->AT.bytes(), mem, k->st); kb_compute_ata(k); }
        if (options & PQ_KKT_UPDATE_G) copy_in(k->GT.p, GT, k->GT.bytes(), mem, k->st);
        stream_wait(k->st);  // host source buffers may be released by the caller after return
        return (int)PQ_OK;
    });
}

int pq_kkt_batch_update_scalings_and_factor(pq_kkt_batch* k, const double* delta, const double* x_reg, const double* z_reg, int mem)
{
    if (!k || !delta || !x_reg || (k->m > 0 && !z_reg)) return fail(PQ_ERR_INVALID, "null argument");
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense KKT batch: bad mem");
    int good = 0;
    const int rc = guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        const int n = k->n, batch = k->batch;
        const auto w0 = std::chrono::steady_clock::now();
        hipStream_t st = k->st;
        size_t off = 0;
        KbFactorArgs a;
        a.n = n; a.p = k->p; a.m = k->m; a.ld = dfb_ld(n); a.width = n < 32 ? n : dfb_block_size_rule(n); a.batch = batch;
        a.Pu = k->Pu.p; a.ATA = k->p > 0 ? k->ATA.p : nullptr; a.GT = k->GT.p;
        a.delta = kb_in(k->stage_in, k->st, delta, (size_t)batch, mem, off);
        a.x_reg = kb_in(k->stage_in, k->st, x_reg, (size_t)batch * n, mem, off);
        a.z_reg = kb_in(k->stage_in, k->st, z_reg, (size_t)batch * k->m, mem, off);
        a.delta_s = k->delta_s.p; a.x_reg_s = k->x_reg_s.p; a.zinv_s = k->zinv_s.p;
        a.F = k->fac.p; a.info = k->status.p; a.badcol = k->status.p + batch;
        const size_t lds = kb_factor_lds_bytes(n);
        PQ_HIP(hipEventRecord(k->ev[0], st));
        if (n < 32) {
            const int grid = div_up(batch, DFB_THREADS / 64);
            if (k->kind == PQ_DENSE_CHOLESKY) k_kb_factor<0, 64><<<grid, DFB_THREADS, lds, st>>>(a);
            else k_kb_factor<1, 64><<<grid, DFB_THREADS, lds, st>>>(a);
        } else {
            if (k->kind == PQ_DENSE_CHOLESKY) k_kb_factor<0, DFB_THREADS><<<batch, DFB_THREADS, lds, st>>>(a);
            else k_kb_factor<1, DFB_THREADS><<<batch, DFB_THREADS, lds, st>>>(a);
        }
        PQ_HIP(hipGetLastError());
        PQ_HIP(hipEventRecord(k->ev[1], st));
        good = kb_factor_done(k, &w0);
        return (int)PQ_OK;
    });
    return rc == PQ_OK ? good : rc;
}

int pq_kkt_batch_info(const pq_kkt_batch* k, int* ok_host, int* first_bad_col_host)
{
    if (!k || !ok_host) return fail(PQ_ERR_INVALID, "null argument");
    if (!k->computed) return fail(PQ_ERR_INVALID, "dense KKT batch: no factorisation yet");
    for (int b = 0; b < k->batch; ++b) {
        ok_host[b] = k->status_h.p[b] == 0;
        if (first_bad_col_host) first_bad_col_host[b] = k->status_h.p[k->batch + b];
    }
    return PQ_OK;
}

int pq_kkt_batch_solve(pq_kkt_batch* k, const double* rhs_x, const double* rhs_y, const double* rhs_z, double* lhs_x, double* lhs_y, double* lhs_z, int mem)
{
    if (!k || !rhs_x || !lhs_x || (k->p > 0 && (!rhs_y || !lhs_y)) || (k->m > 0 && (!rhs_z || !lhs_z))) return fail(PQ_ERR_INVALID, "null argument");
    if (!k->computed) return fail(PQ_ERR_INVALID, "dense KKT batch: solve before update_scalings_and_factor");
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense KKT batch: bad mem");
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        const size_t b = (size_t)k->batch, n = (size_t)k->n, p = (size_t)k->p, m = (size_t)k->m;
        hipStream_t st = k->st;
        size_t off = 0, ooff = 0;
        const bool preload = k->n_ok < k->batch;  // (the blocks of failed instances come back as they went)
        KbSolveArgs a;
        a.n = k->n; a.p = k->p; a.m = k->m; a.ld = dfb_ld(k->n);
        a.AT = k->AT.p; a.GT = k->GT.p; a.F = k->fac.p; a.delta_s = k->delta_s.p; a.zinv_s = k->zinv_s.p; a.info = k->status.p;
        a.rhs_x = kb_in(k->stage_in, k->st, rhs_x, b * n, mem, off);
        a.rhs_y = kb_in(k->stage_in, k->st, rhs_y, b * p, mem, off);
        a.rhs_z = kb_in(k->stage_in, k->st, rhs_z, b * m, mem, off);
        a.lhs_x = kb_out(k->stage_out, k->st, lhs_x, b * n, mem, ooff, preload);
        a.lhs_y = kb_out(k->stage_out, k->st, lhs_y, b * p, mem, ooff, preload);
        a.lhs_z = kb_out(k->stage_out, k->st, lhs_z, b * m, mem, ooff, preload);
        const int threads = k->n <= 64 ? 64 : KB_SOLVE_THREADS;
        PQ_HIP(hipEventRecord(k->ev[2], st));
        if (k->kind == PQ_DENSE_CHOLESKY) k_kb_solve<0><<<k->batch, threads, kb_solve_lds_bytes(k->n), st>>>(a);
        else k_kb_solve<1><<<k->batch, threads, kb_solve_lds_bytes(k->n), st>>>(a);
        PQ_HIP(hipGetLastError());
        PQ_HIP(hipEventRecord(k->ev[3], st));
        kb_back(k->st, lhs_x, a.lhs_x, b * n, mem);
        kb_back(k->st, lhs_y, a.lhs_y, b * p, mem);
        kb_back(k->st, lhs_z, a.lhs_z, b * m, mem);
        stream_wait(st);
        k->timed[1] = true;
        return (int)PQ_OK;
    });
}

int pq_kkt_batch_eval_P_x(pq_kkt_batch* k, const double* alpha, const double* x, double* z, int mem)
{
    if (!k || !alpha || !x || !z) return fail(PQ_ERR_INVALID, "null argument");
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense KKT batch: bad mem");
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        const size_t b = (size_t)k->batch, n = (size_t)k->n;
        size_t off = 0, ooff = 0;
        const double* da = kb_in(k->stage_in, k->st, alpha, b, mem, off);
        const double* dx = kb_in(k->stage_in, k->st, x, b * n, mem, off);
        double* dz = kb_out(k->stage_out, k->st, z, b * n, mem, ooff, false);
        k_kb_eval_P<<<dim3(div_up(k->n, KB_EVAL_THREADS), k->batch), KB_EVAL_THREADS, 0, k->st>>>(k->n, k->Pu.p, da, dx, dz);
        PQ_HIP(hipGetLastError());
        kb_back(k->st, z, dz, b * n, mem);
        stream_wait(k->st);
        return (int)PQ_OK;
    });
}

namespace {
int kb_eval_nt(pq_kkt_batch* k, int cols, const DBuf<double>& M, const double* alpha_n, const double* alpha_t, const double* xn, const double* xt, double* zn,
               double* zt, int mem)
{
    if (!k || !alpha_n || !alpha_t || !xn || !zt || (cols > 0 && (!xt || !zn))) return fail(PQ_ERR_INVALID, "null argument");
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense KKT batch: bad mem");
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        const size_t b = (size_t)k->batch, n = (size_t)k->n, c = (size_t)cols;
        size_t off = 0, ooff = 0;
        const double* dan = kb_in(k->stage_in, k->st, alpha_n, b, mem, off);
        const double* dat = kb_in(k->stage_in, k->st, alpha_t, b, mem, off);
        const double* dxn = kb_in(k->stage_in, k->st, xn, b * n, mem, off);
        const double* dxt = kb_in(k->stage_in, k->st, xt, b * c, mem, off);
        double* dzn = kb_out(k->stage_out, k->st, zn, b * c, mem, ooff, false);
        double* dzt = kb_out(k->stage_out, k->st, zt, b * n, mem, ooff, false);
        k_kb_eval_NT<<<dim3(div_up(k->n + cols, KB_EVAL_THREADS), k->batch), KB_EVAL_THREADS, 0, k->st>>>(k->n, cols, M.p, dan, dat, dxn, dxt, dzn, dzt);
        PQ_HIP(hipGetLastError());
        kb_back(k->st, zn, dzn, b * c, mem);
        kb_back(k->st, zt, dzt, b * n, mem);
        stream_wait(k->st);
        return (int)PQ_OK;
    });
}
}  // namespace

int pq_kkt_batch_eval_A_xn_and_AT_xt(pq_kkt_batch* k, const double* alpha_n, const double* alpha_t, const double* xn, const double* xt, double* zn, double* zt, int mem)
{
    if (!k) return fail(PQ_ERR_INVALID, "null argument");
    return kb_eval_nt(k, k->p, k->AT, alpha_n, alpha_t, xn, xt, zn, zt, mem);
}

int pq_kkt_batch_eval_G_xn_and_GT_xt(pq_kkt_batch* k, const double* alpha_n, const double* alpha_t, const double* xn, const double* xt, double* zn, double* zt, int mem)
{
    if (!k) return fail(PQ_ERR_INVALID, "null argument");
    return kb_eval_nt(k, k->m, k->GT, alpha_n, alpha_t, xn, xt, zn, zt, mem);
}

int pq_kkt_batch_internal_kkt_mat(pq_kkt_batch* k, int instance, double* out_host)
{
    if (!k || !out_host) return fail(PQ_ERR_INVALID, "null argument");
    if (!k->computed) return fail(PQ_ERR_INVALID, "dense KKT batch: no factorisation yet");
    if (instance < 0 || instance >= k->batch) return fail(PQ_ERR_INVALID, "dense KKT batch: instance %d outside [0, %d)", instance, k->batch);
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        const size_t i = (size_t)instance, n = (size_t)k->n, nn = n * n;
        kb_launch_assemble(k, 1, k->m, k->GT.p + i * n * k->m, k->m > 0 ? k->zinv_s.p + i * k->m : nullptr, k->Pu.p + i * nn, k->x_reg_s.p + i * n,
                           k->p > 0 ? k->ATA.p + i * nn : nullptr, k->delta_s.p + i, k->mat_d.p);
        PQ_HIP(hipMemcpyAsync(k->mat_h.p, k->mat_d.p, sizeof(double) * nn, hipMemcpyDeviceToHost, k->st));
        stream_wait(k->st);
        std::memcpy(out_host, k->mat_h.p, sizeof(double) * nn);
        return (int)PQ_OK;
    });
}

int pq_kkt_batch_internal_factor(pq_kkt_batch* k, int instance, double* out_host)
{
    if (!k || !out_host) return fail(PQ_ERR_INVALID, "null argument");
    if (!k->computed) return fail(PQ_ERR_INVALID, "dense KKT batch: no factorisation yet");
    if (instance < 0 || instance >= k->batch) return fail(PQ_ERR_INVALID, "dense KKT batch: instance %d outside [0, %d)", instance, k->batch);
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        const size_t nn = (size_t)k->n * k->n;
        PQ_HIP(hipMemcpyAsync(k->mat_h.p, k->fac.p + (size_t)instance * nn, sizeof(double) * nn, hipMemcpyDeviceToHost, k->st));
        stream_wait(k->st);
        std::memcpy(out_host, k->mat_h.p, sizeof(double) * nn);
        return (int)PQ_OK;
    });
}

int pq_kkt_batch_last_ms(const pq_kkt_batch* k, double out3[3])
{
    if (!k || !out3) return fail(PQ_ERR_INVALID, "null argument");
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        for (int s = 0; s < 2; ++s) {
            float ms = 0.f;
            if (k->timed[s]) PQ_HIP(hipEventElapsedTime(&ms, k->ev[2 * s], k->ev[2 * s + 1]));
            out3[s] = ms;
        }
        out3[2] = k->wall_ms;
        return (int)PQ_OK;
    });
}

}  // extern "C"
