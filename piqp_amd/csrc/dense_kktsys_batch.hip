// piqp_amd/csrc/dense_kktsys_batch.hip -- pq_kktsys_batch_*: piqp::KKTSystem (kkt_system.hpp:97-536) for a BATCH of small dense QPs over the batched dense KKT backend
// (dense_kkt_batch.hip, n <= 128).  Per instance every number is the CPU oracle's (oracle/orc_kkt_system.c over oracle/orc_dense.c) bit for bit.  This file is compiled
// with -ffp-contract=off (piqp_amd/build.py, NO_CONTRACT): the shell's own formulas are those of kkt_system.hip (k_scalings_fused, k_rhs_bars_fused, k_err_x, k_err_yz,
// k_add_inplace, k_dual_recovery, k_box_recovery, k_mul_*), every product and sum rounded on its own; the fused operations are the explicit fma() of the kb_* pieces
// (dense_kkt_batch_device.hpp), which replay the contracted orc_dense.c.
//
//   oracle (orc_kkt_system.c)                 here
//   update_scalings_and_factor :148-199       k_ksb_factor, ONE launch with the backend's launch shape (n >= 32: a workgroup of 256 per instance; n < 32: four instances per
//                                             workgroup, one wave each): the copies and reciprocals, x_reg and z_reg strided over the instance's threads; with the instance's
//                                             refinement flag set max_diag (the |P_jj + x_reg_j| part ignores NaN, a NaN zmax is ignored), reg, delta_reg, x_reg += reg,
//                                             z_reg_iter_ref = z_reg + reg -- both maxima are order-independent, so they are wave / workgroup reductions; then the backend's
//                                             own steps: 1 / z_reg_iter_ref stored, kb_assemble into LDS, dfb_factor_in_lds, the factor to memory.  The backend handle is
//                                             left as pq_kkt_batch_update_scalings_and_factor(delta_reg, x_reg, z_reg_iter_ref) leaves it
//   solve :246-362                            k_ksb_solve, ONE launch, one workgroup per instance, the factor in LDS for the whole launch: rhs_z_bar / rhs_x_bar, the
//                                             backend solve (kb_rhs_row's chain, kb_sweeps, kb_epilogues' formulas), with refinement rhs_norm, get_refine_error and the
//                                             counted loop it < max_iter with its three exits; the pointer swaps of :301,:305 are swaps of workgroup-uniform pointers.
//                                             Without refinement the all-finite check.  Then the dual and box recoveries and the copy of the accepted iterate to lhs
//   mul_condensed_kkt, get_refine_error       ksb_refine_error: kb_eval_P_row, kb_gemv_t_col and the gemv_n chain with alpha = 1.0; m_x_reg includes reg, m_delta and m_z_reg do not
//   inf_norm3 / amax :140-145,:202-208        NaN-sticky workgroup maximum (wave_max_nan of kkt_system.hip)
//   mul :365-394                              k_ksb_mul, one launch, one workgroup per instance
//
// The finite-bound lists: one set for the batch (pq_kktsys_batch_create_dense), or one per instance (pq_kktsys_batch_create_dense_lists, replaced by
// pq_kktsys_batch_set_lists).  The kernels get them as a KbBounds (dense_kkt_batch_device.hpp) and are built twice, template parameter PER: with shared lists the
// six table pointers and the counts are used as they come, as plain arguments were before -- nothing is computed or read per instance, the code is the one of
// before; with lists per instance kb_bound_row moves the pointers to row `inst` of 2 m + 4 n ints and reads cnt_d[4 inst ..].  In the n < 32 variant of k_ksb_factor,
// four instances to a workgroup, row and counts are per wave.  Every loop over a box list runs to the instance's own count.
//
// Memory of the solve kernel: beside the factor and the sweeps' scratch four n-vectors in LDS (lhs_x, ref_lhs_x, err_x, rhs_x_bar): n (n | 1) + 7 n + 2 doubles, 137.0 KiB
// at n = 128.  The p- and m-length vectors (lhs, ref_lhs, err) live in a per-instance workspace in global memory, rhs_z_bar in the handle's state.  What a launch writes
// to global memory and reads again is reached through plain pointers only (the rule above the helpers of dense_kkt_batch_device.hpp), and the phases are separated by
// __syncthreads().  The one exception is the weight vector of kb_assemble (1 / z_reg_iter_ref, written by the factor launch a barrier earlier): its address is per
// lane, a vector load.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "dense_kkt_batch_internal.hpp"

namespace pq {

namespace {

inline size_t ksb_factor_lds_doubles(int n) { return kb_lds_doubles(n) + (size_t)n; }  // the backend's, and x_reg
inline size_t ksb_factor_lds_bytes(int n) { return sizeof(double) * ksb_factor_lds_doubles(n) * (n < 32 ? DFB_THREADS / 64 : 1); }
inline size_t ksb_solve_lds_bytes(int n) { return kb_solve_lds_bytes(n) + sizeof(double) * 4 * (size_t)n; }

// the oracle's amax step: once NaN, NaN
__device__ __forceinline__ double ksb_max_nan(double a, double o) { return (a != a || o != o) ? __builtin_nan("") : (a > o ? a : o); }
__device__ __forceinline__ double ksb_wave_max_nan(double a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a = ksb_max_nan(a, __shfl_xor(a, off, 64));
    return a;
}
// maximum of values that are never NaN
__device__ __forceinline__ double ksb_wave_max(double a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(a, off, 64);
        a = o > a ? o : a;
    }
    return a;
}

// ---- extract_P_diag (kkt_system.hpp:430-453): the diagonal the refinement's max_diag reads is the one of the last update_data that carried P, not the live one
// list: null = every instance; else total = count n and element e belongs to instance list[e / n]
__global__ void k_ksb_pdiag(const double* __restrict__ Pu, double* __restrict__ out, int n, long long total, const int* __restrict__ list)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long long inst = list ? list[e / n] : e / n;
    const int i = (int)(e % n);
    out[inst * n + i] = Pu[inst * (size_t)n * n + i + (size_t)i * n];
}

// ---- update_scalings_and_factor
struct KsbFactorArgs {
    int n, p, m, ld, width, count;  // count: the slots of the grid -- the batch, or the length of `list`
    KbBounds bd;                  // row i has a lower / upper bound (has_* >= 0); variable i is entry pos_* of the lower / upper box list (or -1)
    const double *Pu, *ATA, *GT;  // the backend's data
    const int* flags;             // [batch] or null (off everywhere)
    const int* active;            // [batch] or null (every instance): an instance whose word is 0 is left out -- nothing of it is read or written
    const double *rho, *delta;    // [batch]
    const double *v_s_l, *v_z_l, *v_s_u, *v_z_u, *v_s_bl, *v_z_bl, *v_s_bu, *v_z_bu;  // the caller's state, [batch][m] resp. [batch][n]
    const double* xbs;                         // [batch][n]
    const double* pdiag;                       // [batch][n]: the diagonal of P as of the last update_data that carried P (kkt_system.hpp:134-141)
    double reg_eps, reg_rel;
    double *s_l, *zinv_l, *s_u, *zinv_u, *s_bl, *zinv_bl, *s_bu, *zinv_bu, *z_reg, *rho_s, *mdelta_s;  // the handle's state
    int* use_ref;
    double *delta_s, *x_reg_s, *zinv_s, *F;  // the backend's stored scalings (delta_reg, x_reg with reg, 1 / z_reg_iter_ref) and factor store
    int *info, *badcol;
    const int* list;  // SEL only: slot s works on instance list[s] (distinct entries); every array above is indexed by INSTANCE
};

// SEL = false: slot s of the grid is instance s -- the code of before lists of instances existed (the one read of A.list is not compiled).  SEL = true: the grid is
// sized by the list and a slot learns its instance from it, nothing else differs.
template <int KIND, int G, bool PER, bool SEL>
__global__ __launch_bounds__(DFB_THREADS) void k_ksb_factor(const KsbFactorArgs A)
{
    extern __shared__ double ksb_lds[];
    constexpr int MPW = DFB_THREADS / G, WPG = G / 64;
    __shared__ int s_fail[MPW];
    __shared__ double s_md[DFB_THREADS / 64], s_zm[DFB_THREADS / 64];
    const int n = A.n, m = A.m, ld = A.ld;
    const int g = threadIdx.x / G, t = threadIdx.x % G;
    const long long slot = (long long)blockIdx.x * MPW + g;
    const bool in = slot < A.count;
    // (the slot is the same in every lane of a wave, so the list is read once per wave through a uniform address; without a list the slot is the instance)
    const long long inst = SEL && in ? (long long)A.list[G == 64 ? __builtin_amdgcn_readfirstlane((int)slot) : (int)slot] : slot;
    const bool have = in && (!A.active || A.active[inst] != 0);  // (an instance left out is an empty slot: it still reaches every barrier)
    double* a = ksb_lds + (size_t)g * ((size_t)n * ld + (size_t)(KB_SLICE + 2) * n + KB_SLICE);
    double* dacc = a + (size_t)n * ld;
    double* gs = dacc + n;
    double* ws = gs + (size_t)KB_SLICE * n;
    double* xr = ws + KB_SLICE;  // x_reg of this instance
    if (t == 0) s_fail[g] = -1;
    const size_t nn = (size_t)n * n, om = have ? (size_t)inst * m : 0, on = have ? (size_t)inst * n : 0;
    double* z_reg = A.z_reg + om;  // (written and read again below: a plain pointer)
    double rho = 0.0, delta = 1.0, md = 0.0, zm = 0.0;
    if (have) {
        // (the instance is the same in every lane of a wave: with G == 64 the table row and the counts are per wave, not per workgroup)
        const KbBounds R = kb_bound_row<PER>(A.bd, G == 64 ? (long long)__builtin_amdgcn_readfirstlane((int)inst) : inst);
        rho = A.rho[inst];
        delta = A.delta[inst];
        // kkt_system.hpp:150-193, the formulas of k_scalings_fused
        for (int i = t; i < m; i += G) {
            const double sl = A.v_s_l[om + i], zil = 1.0 / A.v_z_l[om + i], su = A.v_s_u[om + i], ziu = 1.0 / A.v_z_u[om + i];
            A.s_l[om + i] = sl; A.zinv_l[om + i] = zil; A.s_u[om + i] = su; A.zinv_u[om + i] = ziu;
            double v = 0.0;
            if (R.has_l[i] >= 0) v += 1.0 / (zil * sl + delta);
            if (R.has_u[i] >= 0) v += 1.0 / (ziu * su + delta);
            v = 1.0 / v;
            z_reg[i] = v;
            zm = ksb_max_nan(zm, fabs(v));
        }
        for (int i = t; i < R.nxl; i += G) { A.s_bl[on + i] = A.v_s_bl[on + i]; A.zinv_bl[on + i] = 1.0 / A.v_z_bl[on + i]; }
        for (int i = t; i < R.nxu; i += G) { A.s_bu[on + i] = A.v_s_bu[on + i]; A.zinv_bu[on + i] = 1.0 / A.v_z_bu[on + i]; }
        for (int i = t; i < n; i += G) {
            double v = rho;
            const double sc = A.xbs[on + i];
            const int il = R.pos_l[i], iu = R.pos_u[i];
            if (il >= 0) v += sc * sc / ((1.0 / A.v_z_bl[on + il]) * A.v_s_bl[on + il] + delta);
            if (iu >= 0) v += sc * sc / ((1.0 / A.v_z_bu[on + iu]) * A.v_s_bu[on + iu] + delta);
            xr[i] = v;
            const double d = fabs(A.pdiag[on + i] + v);
            if (d > md) md = d;  // (a NaN is ignored)
        }
    }
    md = ksb_wave_max(md);
    zm = ksb_wave_max_nan(zm);
    if ((threadIdx.x & 63) == 0) { s_md[threadIdx.x >> 6] = md; s_zm[threadIdx.x >> 6] = zm; }
    __syncthreads();
    md = s_md[g * WPG];
    zm = s_zm[g * WPG];
#pragma unroll
    for (int w = 1; w < WPG; ++w) {
        md = s_md[g * WPG + w] > md ? s_md[g * WPG + w] : md;
        zm = ksb_max_nan(zm, s_zm[g * WPG + w]);
    }
    // kkt_system.hpp:195-207
    double delta_reg = delta;
    if (have) {
        const bool flag = A.flags && A.flags[inst] != 0;
        double reg = 0.0;
        if (flag) {
            if (zm > md) md = zm;  // (a NaN zmax is ignored)
            reg = A.reg_eps + A.reg_rel * md;
            delta_reg = delta + reg;
        }
        for (int i = t; i < n; i += G) {
            double v = xr[i];
            if (flag) v = v + reg;
            xr[i] = v;
            A.x_reg_s[on + i] = v;
        }
        for (int k = t; k < m; k += G) {  // (entry k was written by this very thread)
            double v = z_reg[k];
            if (flag) v = v + reg;
            A.zinv_s[om + k] = 1.0 / v;
        }
        if (t == 0) { A.delta_s[inst] = delta_reg; A.rho_s[inst] = rho; A.mdelta_s[inst] = delta; A.use_ref[inst] = flag ? 1 : 0; }
    }
    __syncthreads();
    // the backend's update_scalings_and_factor from here on (k_kb_factor)
    const double dinv = 1.0 / delta_reg;
    kb_assemble<G>(a, dacc, gs, ws, n, ld, m, have ? A.GT + inst * (size_t)n * m : nullptr, have && m > 0 ? A.zinv_s + om : nullptr, false, have ? A.Pu + inst * nn : nullptr, xr,
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

// ---- solve
// NaN-sticky maximum over the workgroup; red: one double per wave (LDS).  Called by the whole workgroup; every thread gets the result.
__device__ __forceinline__ double ksb_block_max_nan(double v, double* red)
{
    v = ksb_wave_max_nan(v);
    __syncthreads();  // (the result before has been read)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = ksb_max_nan(r, red[w]);
    return r;
}

struct KsbSolveArgs {
    int n, p, m, ld, max_iter, batch;
    KbBounds bd;
    double eps_abs, eps_rel, min_rate;
    const double *Pu, *AT, *GT, *F, *delta_s, *x_reg_s, *zinv_s;  // the backend's data, stored scalings and factors
    const int* info;
    const int* active;  // [batch] or null (every instance): the workgroup of an instance whose word is 0 returns at once
    const double *s_l, *zinv_l, *s_u, *zinv_u, *s_bl, *zinv_bl, *s_bu, *zinv_bu, *z_reg, *mdelta_s, *xbs;  // the state of the last update_scalings_and_factor
    const int* use_ref;
    pq_vars rhs, lhs;                // [batch][len] each; rhs is only read
    double *rhs_x_bar, *rhs_z_bar;   // state: [batch][n], [batch][m]
    double *wy, *wz;                 // workspace: [batch][3][p], [batch][3][m] (lhs, ref_lhs, err)
    int* sinfo;                      // [3][batch]: solve_ok, refine steps, backend solves
    double* dinfo;                   // [2][batch]: refine error, rhs norm
    const int* list;                 // SEL only: the grid has one workgroup per entry and workgroup s works on instance list[s]
};

// what one instance's workgroup keeps at hand
struct KsbInst {
    int n, p, m, ld, t, T;
    const double *a, *Pu, *AT, *GT, *zinv, *x_reg, *z_reg, *rhs_y;
    double dinv, mdelta;
    double *xs, *pr, *xb, *red;
    const double* rxb;  // LDS
    const double* rzb;  // global, written by this launch
};

// dense_solve (orc_dense.c:672-688) of one instance.  rx, ox: LDS; ry, rz, oy, oz: global, plain.  Barriers on entry and on return.
template <int KIND>
__device__ __forceinline__ void ksb_backend_solve(const KsbInst& I, const double* rx, const double* ry, const double* rz, double* ox, double* oy, double* oz)
{
    __syncthreads();
    double c = 0.0;
    if (I.t < I.n) c = kb_rhs_row(I.t, I.n, I.p, I.m, I.GT, I.AT, I.zinv, I.dinv, rx, ry, rz);
    kb_sweeps<KIND>(I.a, I.n, I.ld, c, I.xs, I.pr, I.xb, I.t);
    if (I.t < I.n) ox[I.t] = I.xs[I.t];
    kb_epilogues(I.n, I.p, I.m, I.GT, I.AT, I.zinv, I.dinv, I.xs, ry, rz, oy, oz, I.t, I.T);
    __syncthreads();
}

// get_refine_error :227-236 over mul_condensed_kkt :211-224 (k_err_x, k_err_yz): err = rhs_bar - K_cond lhs, returns its NaN-sticky inf-norm
__device__ __forceinline__ double ksb_refine_error(const KsbInst& I, const double* lx, const double* ly, const double* lz, double* ex, double* ey, double* ez)
{
    __syncthreads();
    const int n = I.n, t = I.t;
    double nrm = 0.0;
    if (t < n) {
        double v = kb_eval_P_row(t, n, I.Pu, 1.0, lx);
        v = v + I.x_reg[t] * lx[t];
        v = v + kb_gemv_n_row(t, n, I.p, I.AT, ly, 1.0);
        v = v + kb_gemv_n_row(t, n, I.m, I.GT, lz, 1.0);
        const double e = I.rxb[t] - v;
        ex[t] = e;
        nrm = ksb_max_nan(nrm, fabs(e));
    }
    for (int j = t; j < I.p; j += I.T) {
        double v = kb_gemv_t_col(j, n, I.AT, lx, 1.0);
        v = v - I.mdelta * ly[j];
        const double e = I.rhs_y[j] - v;
        ey[j] = e;
        nrm = ksb_max_nan(nrm, fabs(e));
    }
    for (int j = t; j < I.m; j += I.T) {
        double v = kb_gemv_t_col(j, n, I.GT, lx, 1.0);
        v = v - I.z_reg[j] * lz[j];
        const double e = I.rzb[j] - v;
        ez[j] = e;
        nrm = ksb_max_nan(nrm, fabs(e));
    }
    return ksb_block_max_nan(nrm, I.red);
}

__device__ __forceinline__ void ksb_swap(double*& a, double*& b) { double* c = a; a = b; b = c; }

template <int KIND, bool PER, bool SEL>  // (SEL: as at k_ksb_factor)
__global__ __launch_bounds__(KB_SOLVE_THREADS) void k_ksb_solve(const KsbSolveArgs A)
{
    extern __shared__ double ksb_lds[];
    __shared__ double s_red[KB_SOLVE_THREADS / 64];
    const long long inst = SEL ? (long long)A.list[blockIdx.x] : (long long)blockIdx.x;  // (one scalar read per workgroup)
    const int n = A.n, p = A.p, m = A.m, ld = A.ld, t = threadIdx.x, T = blockDim.x;
    if (A.active && A.active[inst] == 0) return;  // (uniform: before any barrier)
    if (A.info[inst] != 0) {  // (uniform: before any barrier) the factorisation failed: the lhs blocks are not touched
        if (t == 0) {
            A.sinfo[inst] = 0; A.sinfo[A.batch + inst] = 0; A.sinfo[2 * (size_t)A.batch + inst] = 0;
            A.dinfo[inst] = 0.0; A.dinfo[A.batch + inst] = 0.0;
        }
        return;
    }
    double* a = ksb_lds;
    double* xs = a + (size_t)n * ld;
    double* pr = xs + n;
    double* xb = pr + 2 * (size_t)n;
    double* lx = xb + 2;  // lhs_x
    double* rlx = lx + n;  // ref_lhs_x
    double* ex = rlx + n;  // err_x
    double* rxb = ex + n;  // rhs_x_bar
    const double* src = A.F + inst * (size_t)n * n;
    for (int e = t; e < n * n; e += T) {
        const int j = e / n, i = e % n;
        if (i >= j) a[i + j * ld] = src[e];
    }
    const size_t om = (size_t)inst * m, on = (size_t)inst * n, op = (size_t)inst * p;
    const KbBounds R = kb_bound_row<PER>(A.bd, inst);
    const double delta = A.mdelta_s[inst];
    double* rzb = A.rhs_z_bar + om;
    double *ly = A.wy + 3 * op, *rly = ly + p, *ey = rly + p;
    double *lz = A.wz + 3 * om, *rlz = lz + m, *ez = rlz + m;
    // kkt_system.hpp:219-252, the formulas of k_rhs_bars_fused
    {
        const double *s_l = A.s_l + om, *zinv_l = A.zinv_l + om, *s_u = A.s_u + om, *zinv_u = A.zinv_u + om, *z_reg = A.z_reg + om;
        const double *r_z_l = A.rhs.z_l + om, *r_s_l = A.rhs.s_l + om, *r_z_u = A.rhs.z_u + om, *r_s_u = A.rhs.s_u + om;
        for (int i = t; i < m; i += T) {
            double v = 0.0;
            if (R.has_l[i] >= 0) v -= 1.0 / (zinv_l[i] * s_l[i] + delta) * (r_z_l[i] - zinv_l[i] * r_s_l[i]);
            if (R.has_u[i] >= 0) v += 1.0 / (zinv_u[i] * s_u[i] + delta) * (r_z_u[i] - zinv_u[i] * r_s_u[i]);
            rzb[i] = v * z_reg[i];
        }
        const double *s_bl = A.s_bl + on, *zinv_bl = A.zinv_bl + on, *s_bu = A.s_bu + on, *zinv_bu = A.zinv_bu + on, *xbs = A.xbs + on;
        const double *r_z_bl = A.rhs.z_bl + on, *r_s_bl = A.rhs.s_bl + on, *r_z_bu = A.rhs.z_bu + on, *r_s_bu = A.rhs.s_bu + on;
        for (int i = t; i < n; i += T) {
            double v = A.rhs.x[on + i];
            const int il = R.pos_l[i], iu = R.pos_u[i];
            if (il >= 0) v -= xbs[i] * (r_z_bl[il] - zinv_bl[il] * r_s_bl[il]) / (s_bl[il] * zinv_bl[il] + delta);
            if (iu >= 0) v += xbs[i] * (r_z_bu[iu] - zinv_bu[iu] * r_s_bu[iu]) / (s_bu[iu] * zinv_bu[iu] + delta);
            rxb[i] = v;
            A.rhs_x_bar[on + i] = v;
        }
    }
    KsbInst I;
    I.n = n; I.p = p; I.m = m; I.ld = ld; I.t = t; I.T = T;
    I.a = a; I.Pu = A.Pu + inst * (size_t)n * n; I.AT = A.AT + inst * (size_t)n * p; I.GT = A.GT + inst * (size_t)n * m;
    I.zinv = A.zinv_s + om; I.x_reg = A.x_reg_s + on; I.z_reg = A.z_reg + om; I.rhs_y = A.rhs.y + op;
    I.dinv = 1.0 / A.delta_s[inst]; I.mdelta = delta;
    I.xs = xs; I.pr = pr; I.xb = xb; I.red = s_red; I.rxb = rxb; I.rzb = rzb;

    ksb_backend_solve<KIND>(I, rxb, I.rhs_y, rzb, lx, ly, lz);
    int ok = 1, steps = 0, solves = 1;
    double err = 0.0, rhs_norm = 0.0;
    if (A.use_ref[inst] != 0) {  // kkt_system.hpp:256-301; err and rhs_norm are the same in every thread, so every branch below is uniform
        double v = 0.0;
        if (t < n) v = ksb_max_nan(v, fabs(rxb[t]));
        for (int j = t; j < p; j += T) v = ksb_max_nan(v, fabs(I.rhs_y[j]));
        for (int j = t; j < m; j += T) v = ksb_max_nan(v, fabs(rzb[j]));
        rhs_norm = ksb_block_max_nan(v, s_red);
        err = ksb_refine_error(I, lx, ly, lz, ex, ey, ez);
        if (!isfinite(err)) ok = 0;
        for (int it = 0; ok && it < A.max_iter; ++it) {
            if (err <= A.eps_abs + A.eps_rel * rhs_norm) break;
            const double prev = err;
            ksb_backend_solve<KIND>(I, ex, ey, ez, rlx, rly, rlz);
            ++solves;
            ++steps;
            if (t < n) rlx[t] += lx[t];
            for (int j = t; j < p; j += T) rly[j] += ly[j];
            for (int j = t; j < m; j += T) rlz[j] += lz[j];
            err = ksb_refine_error(I, rlx, rly, rlz, ex, ey, ez);
            if (!isfinite(err)) { ok = 0; break; }
            const double rate = prev / err;
            if (rate < A.min_rate) {
                if (rate > 1.0) { ksb_swap(lx, rlx); ksb_swap(ly, rly); ksb_swap(lz, rlz); }
                break;
            }
            ksb_swap(lx, rlx); ksb_swap(ly, rly); ksb_swap(lz, rlz);
        }
    } else {  // :305 allFinite
        double v = 0.0;
        if (t < n) v = ksb_max_nan(v, fabs(lx[t]));
        for (int j = t; j < p; j += T) v = ksb_max_nan(v, fabs(ly[j]));
        for (int j = t; j < m; j += T) v = ksb_max_nan(v, fabs(lz[j]));
        if (!isfinite(ksb_block_max_nan(v, s_red))) ok = 0;
    }
    if (t == 0) {
        A.sinfo[inst] = ok; A.sinfo[A.batch + inst] = steps; A.sinfo[2 * (size_t)A.batch + inst] = solves;
        A.dinfo[inst] = err; A.dinfo[A.batch + inst] = rhs_norm;
    }
    if (!ok) return;
    __syncthreads();
    // kkt_system.hpp:310-345, k_dual_recovery
    {
        const double *s_l = A.s_l + om, *zinv_l = A.zinv_l + om, *s_u = A.s_u + om, *zinv_u = A.zinv_u + om, *z_reg = A.z_reg + om;
        const double *r_z_l = A.rhs.z_l + om, *r_s_l = A.rhs.s_l + om, *r_z_u = A.rhs.z_u + om, *r_s_u = A.rhs.s_u + om;
        for (int i = t; i < m; i += T) {
            const bool l = R.has_l[i] >= 0, u = R.has_u[i] >= 0;
            double zl = 0.0, zu = 0.0, sl = 0.0, su = 0.0;
            if (l && u) {
                const double rz_l_bar = r_z_l[i] - zinv_l[i] * r_s_l[i];
                const double W_l_inv = 1.0 / (zinv_l[i] * s_l[i] + delta);
                const double rz_u_bar = r_z_u[i] - zinv_u[i] * r_s_u[i];
                const double W_u_inv = 1.0 / (zinv_u[i] * s_u[i] + delta);
                const double r_sum = W_l_inv * W_u_inv * (rz_l_bar + rz_u_bar);
                zl = -z_reg[i] * (r_sum + W_l_inv * lz[i]);
                zu = -z_reg[i] * (r_sum - W_u_inv * lz[i]);
                sl = zinv_l[i] * (r_s_l[i] - s_l[i] * zl);
                su = zinv_u[i] * (r_s_u[i] - s_u[i] * zu);
            } else if (l) {
                zl = -lz[i];
                sl = zinv_l[i] * (r_s_l[i] - s_l[i] * zl);
            } else if (u) {
                zu = lz[i];
                su = zinv_u[i] * (r_s_u[i] - s_u[i] * zu);
            }
            A.lhs.z_l[om + i] = zl; A.lhs.z_u[om + i] = zu; A.lhs.s_l[om + i] = sl; A.lhs.s_u[om + i] = su;
        }
    }
    // :347-366, k_box_recovery
    {
        const double* xbs = A.xbs + on;
        for (int i = t; i < R.nxl; i += T) {
            const int idx = R.xl_idx[i];
            const double zinv = A.zinv_bl[on + i], s = A.s_bl[on + i], r_s = A.rhs.s_bl[on + i];
            const double zb = (-1.0 * xbs[idx] * lx[idx] - A.rhs.z_bl[on + i] + zinv * r_s) / (s * zinv + delta);
            A.lhs.z_bl[on + i] = zb;
            A.lhs.s_bl[on + i] = zinv * (r_s - s * zb);
        }
        for (int i = t; i < R.nxu; i += T) {
            const int idx = R.xu_idx[i];
            const double zinv = A.zinv_bu[on + i], s = A.s_bu[on + i], r_s = A.rhs.s_bu[on + i];
            const double zb = (1.0 * xbs[idx] * lx[idx] - A.rhs.z_bu[on + i] + zinv * r_s) / (s * zinv + delta);
            A.lhs.z_bu[on + i] = zb;
            A.lhs.s_bu[on + i] = zinv * (r_s - s * zb);
        }
    }
    for (int i = t; i < n; i += T) A.lhs.x[on + i] = lx[i];
    for (int j = t; j < p; j += T) A.lhs.y[op + j] = ly[j];
}

// ---- mul
struct KsbMulArgs {
    int n, p, m;
    KbBounds bd;
    const double *Pu, *AT, *GT;
    const double *s_l, *zinv_l, *s_u, *zinv_u, *s_bl, *zinv_bl, *s_bu, *zinv_bu, *rho_s, *mdelta_s, *xbs;
    pq_vars lhs, rhs;  // lhs is only read
    double* wz;        // [batch][3][m]: the first m of an instance hold z_u - z_l
};

// kkt_system.hpp:392-425 (k_mul_x, k_mul_y, k_mul_z, k_mul_box): blockIdx.x = instance
template <bool PER>
__global__ __launch_bounds__(KB_SOLVE_THREADS) void k_ksb_mul(const KsbMulArgs A)
{
    const long long inst = blockIdx.x;
    const int n = A.n, p = A.p, m = A.m, t = threadIdx.x, T = blockDim.x;
    const size_t om = (size_t)inst * m, on = (size_t)inst * n, op = (size_t)inst * p;
    const double rho = A.rho_s[inst], delta = A.mdelta_s[inst];
    const KbBounds R = kb_bound_row<PER>(A.bd, inst);
    const double *Pu = A.Pu + inst * (size_t)n * n, *AT = A.AT + inst * (size_t)n * p, *GT = A.GT + inst * (size_t)n * m, *xbs = A.xbs + on;
    const double *lx = A.lhs.x + on, *ly = A.lhs.y + op, *z_l = A.lhs.z_l + om, *z_u = A.lhs.z_u + om, *s_l = A.lhs.s_l + om, *s_u = A.lhs.s_u + om;
    const double *z_bl = A.lhs.z_bl + on, *z_bu = A.lhs.z_bu + on, *s_bl = A.lhs.s_bl + on, *s_bu = A.lhs.s_bu + on;
    double* d = A.wz + 3 * om;  // (written here, read below: a plain pointer)
    for (int j = t; j < m; j += T) d[j] = z_u[j] - z_l[j];
    __syncthreads();
    for (int i = t; i < n; i += T) {
        double v = kb_eval_P_row(i, n, Pu, 1.0, lx);
        v = v + rho * lx[i];
        v = v + kb_gemv_n_row(i, n, p, AT, ly, 1.0);
        v = v + kb_gemv_n_row(i, n, m, GT, d, 1.0);
        if (R.pos_l[i] >= 0) v = v - xbs[i] * z_bl[R.pos_l[i]];
        if (R.pos_u[i] >= 0) v = v + xbs[i] * z_bu[R.pos_u[i]];
        A.rhs.x[on + i] = v;
    }
    for (int j = t; j < p; j += T) A.rhs.y[op + j] = kb_gemv_t_col(j, n, AT, lx, 1.0) - delta * ly[j];
    for (int j = t; j < m; j += T) {
        const double Gx = kb_gemv_t_col(j, n, GT, lx, 1.0);
        A.rhs.z_l[om + j] = -Gx + (s_l[j] - delta * z_l[j]);
        A.rhs.z_u[om + j] = Gx + (s_u[j] - delta * z_u[j]);
        A.rhs.s_l[om + j] = A.s_l[om + j] * z_l[j] + s_l[j] / A.zinv_l[om + j];
        A.rhs.s_u[om + j] = A.s_u[om + j] * z_u[j] + s_u[j] / A.zinv_u[om + j];
    }
    for (int i = t; i < R.nxl; i += T) {
        const int idx = R.xl_idx[i];
        A.rhs.z_bl[on + i] = -1.0 * xbs[idx] * lx[idx] - delta * z_bl[i] + s_bl[i];
        A.rhs.s_bl[on + i] = A.s_bl[on + i] * z_bl[i] + s_bl[i] / A.zinv_bl[on + i];
    }
    for (int i = t; i < R.nxu; i += T) {
        const int idx = R.xu_idx[i];
        A.rhs.z_bu[on + i] = 1.0 * xbs[idx] * lx[idx] - delta * z_bu[i] + s_bu[i];
        A.rhs.s_bu[on + i] = A.s_bu[on + i] * z_bu[i] + s_bu[i] / A.zinv_bu[on + i];
    }
}

}  // namespace

}  // namespace pq

using namespace pq;

namespace {
// the state vectors of a handle, [batch][len] each
enum { S_SL, S_ZIL, S_SU, S_ZIU, S_SBL, S_ZIBL, S_SBU, S_ZIBU, S_ZREG, S_RHO, S_MDELTA, S_RXB, S_RZB, S_XBS, S_PDIAG, S_COUNT };
struct KbDeleter {
    void operator()(pq_kkt_batch* b) const { pq_kkt_batch_destroy(b); }
};
}  // namespace

struct pq_kktsys_batch {
    int device = 0, batch = 0, n = 0, p = 0, m = 0;
    bool per_inst = false;           // every instance has lists of its own (pq_kktsys_batch_create_dense_lists)
    int cnt[4] = {0, 0, 0, 0};       // n_h_l, n_h_u, n_x_l, n_x_u; per instance: the largest of the batch (is a box vector used at all)
    int box_min[2] = {0, 0};         // the smallest n_x_l, n_x_u of the batch (has a box row an unused tail)
    std::vector<int> idx[4];         // shared: the four lists (host)
    std::vector<int> tab_h, cnt_h;   // per instance: the host images of tab and cnt_d, sized at creation (pq_kktsys_batch_set_lists allocates nothing)
    std::vector<char> seen;          // [m]: scratch of the checks
    pq_settings settings;
    int n_solved = 0;
    bool solved = false, timed[2] = {false, false};
    bool stale = false;              // the lists were replaced after the last factorisation (pq_kktsys_batch_set_lists): as before the first one
    DBuf<double> state[S_COUNT];
    DBuf<int> tab;                   // shared: has_l[m], has_u[m], pos_l[n], pos_u[n], x_l_idx[n_x_l], x_u_idx[n_x_u]; per instance: [batch] rows of 2 m + 4 n (KbBounds)
    DBuf<int> cnt_d;                 // per instance: [batch][4]
    DBuf<int> use_ref, flags_d, sinfo;
    DBuf<double> dinfo, wy, wz, stage_in, stage_out;
    HBuf<int> sinfo_h;
    HBuf<double> dinfo_h;
    Event ev[4];                     // solve begin / end, mul begin / end (the factor launch is timed by the backend's events)
    std::unique_ptr<pq_kkt_batch, KbDeleter> kb;  // last: destroyed first, which drains the one stream everything here runs on
};

namespace {

size_t ksb_state_len(const pq_kktsys_batch* k, int s)
{
    switch (s) {
    case S_SL: case S_ZIL: case S_SU: case S_ZIU: case S_ZREG: case S_RZB: return (size_t)k->m;
    case S_RHO: case S_MDELTA: return 1;
    default: return (size_t)k->n;
    }
}

// the doubles of the ten vectors of a pq_vars that this handle reads / writes (batch x length; 0: the vector has no meaningful part).  first: the positions
// before it count as unused (x and y are not part of a state)
void ksb_var_counts(const pq_kktsys_batch* k, int first, size_t count[10])
{
    vars_lens((size_t)k->n, (size_t)k->p, (size_t)k->m, count);
    for (int i = 0; i < 10; ++i) count[i] = i < first ? 0 : count[i] * (size_t)k->batch;
    if (k->cnt[2] == 0) count[4] = count[8] = 0;  // z_bl, s_bl
    if (k->cnt[3] == 0) count[5] = count[9] = 0;  // z_bu, s_bu
}
double** ksb_fields(pq_vars* v) { return &v->x; }  // (ten pointers in the header's order)
double* const* ksb_fields(const pq_vars* v) { return &v->x; }

int ksb_check_vars(const pq_kktsys_batch* k, const pq_vars* v, int first, const char* what)
{
    size_t count[10];
    ksb_var_counts(k, first, count);
    for (int i = first; i < 10; ++i)
        if (count[i] && !ksb_fields(v)[i]) return fail(PQ_ERR_INVALID, "dense KKT system batch: %s: null vector (position %d of pq_vars)", what, i);
    return PQ_OK;
}

// inputs of a call in device memory: the caller's pointers, or copies in the input staging
pq_vars ksb_vars_in(pq_kktsys_batch* k, const pq_vars* v, int first, int mem, size_t& off)
{
    size_t count[10];
    ksb_var_counts(k, first, count);
    pq_vars d;
    for (int i = 0; i < 10; ++i) ksb_fields(&d)[i] = const_cast<double*>(kb_in(k->stage_in, k->kb->st, ksb_fields(v)[i], count[i], mem, off));
    return d;
}
// outputs: the caller's pointers, or places in the output staging.  Host mode: a block the launch may leave alone (an instance that failed; the unused tail of a box
// row) goes there with the host's present values first
pq_vars ksb_vars_out(pq_kktsys_batch* k, pq_vars* v, int mem, bool preload_all)
{
    size_t count[10], off = 0;
    ksb_var_counts(k, 0, count);
    pq_vars d;
    for (int i = 0; i < 10; ++i) {
        const bool box_tail = ((i == 4 || i == 8) && k->box_min[0] < k->n) || ((i == 5 || i == 9) && k->box_min[1] < k->n);
        ksb_fields(&d)[i] = kb_out(k->stage_out, k->kb->st, ksb_fields(v)[i], count[i], mem, off, preload_all || box_tail);
    }
    return d;
}
void ksb_vars_back(pq_kktsys_batch* k, pq_vars* host, const pq_vars& dev, int mem)
{
    size_t count[10];
    ksb_var_counts(k, 0, count);
    for (int i = 0; i < 10; ++i) kb_back(k->kb->st, ksb_fields(host)[i], ksb_fields(&dev)[i], count[i], mem);
}

void ksb_raise_lds()
{
    static PerDeviceOnce once;
    once([&] {
        const int fb = (int)ksb_factor_lds_bytes(PQ_KKT_BATCH_DENSE_MAX_N), sb = (int)ksb_solve_lds_bytes(PQ_KKT_BATCH_DENSE_MAX_N);
        const void* const factor[8] = {(const void*)k_ksb_factor<0, DFB_THREADS, false, false>, (const void*)k_ksb_factor<1, DFB_THREADS, false, false>,
                                       (const void*)k_ksb_factor<0, DFB_THREADS, true, false>,  (const void*)k_ksb_factor<1, DFB_THREADS, true, false>,
                                       (const void*)k_ksb_factor<0, DFB_THREADS, false, true>,  (const void*)k_ksb_factor<1, DFB_THREADS, false, true>,
                                       (const void*)k_ksb_factor<0, DFB_THREADS, true, true>,   (const void*)k_ksb_factor<1, DFB_THREADS, true, true>};
        const void* const solve[8] = {(const void*)k_ksb_solve<0, false, false>, (const void*)k_ksb_solve<1, false, false>, (const void*)k_ksb_solve<0, true, false>,
                                      (const void*)k_ksb_solve<1, true, false>,  (const void*)k_ksb_solve<0, false, true>,  (const void*)k_ksb_solve<1, false, true>,
                                      (const void*)k_ksb_solve<0, true, true>,   (const void*)k_ksb_solve<1, true, true>};
        for (const void* fn : factor) PQ_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, fb));
        for (const void* fn : solve) PQ_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, sb));
    });
}

// everything but the backend; the backend (k->kb) exists already: its stream carries the memsets
void ksb_alloc(pq_kktsys_batch* k)
{
    const size_t b = (size_t)k->batch, n = (size_t)k->n, p = (size_t)k->p, m = (size_t)k->m;
    hipStream_t st = k->kb->st;
    for (int s = 0; s < S_COUNT; ++s) { k->state[s].alloc(b * ksb_state_len(k, s)); k->state[s].zero(st); }
    if (k->per_inst) { k->tab.alloc(b * (2 * m + 4 * n)); k->cnt_d.alloc(4 * b); }
    else k->tab.alloc(2 * m + 2 * n + (size_t)k->cnt[2] + (size_t)k->cnt[3]);
    k->use_ref.alloc(b); k->use_ref.zero(st);
    k->flags_d.alloc(b);
    k->sinfo.alloc(3 * b); k->sinfo.zero(st);
    k->dinfo.alloc(2 * b); k->dinfo.zero(st);
    k->wy.alloc(3 * b * p); k->wz.alloc(3 * b * m);
    k->stage_in.alloc(b * (5 * n + p + 4 * m + 2)); k->stage_out.alloc(b * (5 * n + p + 4 * m));
    k->sinfo_h.alloc(3 * b); k->dinfo_h.alloc(2 * b);
    std::memset(k->sinfo_h.p, 0, sizeof(int) * 3 * b);
    std::memset(k->dinfo_h.p, 0, sizeof(double) * 2 * b);
    for (Event& e : k->ev) e = Event(0);
    ksb_raise_lds();
}

// has_l, has_u, pos_l, pos_u and the two box lists, from the host lists, to the device (the host vector is read by the time this returns)
void ksb_upload_tables(pq_kktsys_batch* k)
{
    const int n = k->n, m = k->m;
    if (k->per_inst) {  // (the images were filled by ksb_take_lists)
        PQ_HIP(hipMemcpyAsync(k->tab.p, k->tab_h.data(), sizeof(int) * k->tab_h.size(), hipMemcpyHostToDevice, k->kb->st));
        PQ_HIP(hipMemcpyAsync(k->cnt_d.p, k->cnt_h.data(), sizeof(int) * k->cnt_h.size(), hipMemcpyHostToDevice, k->kb->st));
        stream_wait(k->kb->st);
        return;
    }
    std::vector<int> t((size_t)2 * m + 2 * n + k->cnt[2] + k->cnt[3], -1);
    for (int i = 0; i < k->cnt[0]; ++i) t[k->idx[0][i]] = i;
    for (int i = 0; i < k->cnt[1]; ++i) t[(size_t)m + k->idx[1][i]] = i;
    for (int i = 0; i < k->cnt[2]; ++i) { t[(size_t)2 * m + k->idx[2][i]] = i; t[(size_t)2 * m + 2 * n + i] = k->idx[2][i]; }
    for (int i = 0; i < k->cnt[3]; ++i) { t[(size_t)2 * m + n + k->idx[3][i]] = i; t[(size_t)2 * m + 2 * n + k->cnt[2] + i] = k->idx[3][i]; }
    PQ_HIP(hipMemcpyAsync(k->tab.p, t.data(), sizeof(int) * t.size(), hipMemcpyHostToDevice, k->kb->st));
    stream_wait(k->kb->st);
}
// P_diag of every instance from the backend's P, on the handle's stream (nothing waits)
void ksb_extract_pdiag(pq_kktsys_batch* k, const int* list = nullptr, int count = 0)
{
    const long long total = (long long)(list ? count : k->batch) * k->n;
    k_ksb_pdiag<<<(unsigned)((total + 255) / 256), 256, 0, k->kb->st>>>(k->kb->Pu.p, k->state[S_PDIAG].p, k->n, total, list);
    PQ_HIP(hipGetLastError());
}
KbBounds ksb_bounds(const pq_kktsys_batch* k)
{
    const size_t m = (size_t)k->m, n = (size_t)k->n;
    KbBounds b;
    b.has_l = k->tab.p; b.has_u = b.has_l + m; b.pos_l = b.has_u + m; b.pos_u = b.pos_l + n; b.xl_idx = b.pos_u + n;
    b.xu_idx = b.xl_idx + (k->per_inst ? n : (size_t)k->cnt[2]);
    b.nhl = k->cnt[0]; b.nhu = k->cnt[1]; b.nxl = k->cnt[2]; b.nxu = k->cnt[3];
    b.cnt = k->per_inst ? k->cnt_d.p : nullptr;
    b.stride = k->per_inst ? (int)(2 * m + 4 * n) : 0;
    return b;
}

int ksb_check_settings(const pq_settings* s)
{
    if (!s) return fail(PQ_ERR_INVALID, "dense KKT system batch: null settings");
    if (s->iterative_refinement_max_iter < 0 || s->iterative_refinement_max_iter > KB_MAX_REFINE_ITER)
        return fail(PQ_ERR_INVALID, "dense KKT system batch: iterative_refinement_max_iter = %d, [0, %d] wanted (the loop runs inside a kernel)", s->iterative_refinement_max_iter,
                    KB_MAX_REFINE_ITER);
    return PQ_OK;
}

// who: "" for the lists a batch shares, "instance 12: " for those of one instance
int ksb_check_list(const char* who, const char* name, int cnt, const int* idx, int len)
{
    if (cnt < 0) return fail(PQ_ERR_INVALID, "dense KKT system batch: %sn_%s = %d is negative", who, name, cnt);
    if (cnt > len) return fail(PQ_ERR_INVALID, "dense KKT system batch: %sn_%s = %d, its vector has %d entries", who, name, cnt, len);
    if (cnt > 0 && !idx) return fail(PQ_ERR_INVALID, "dense KKT system batch: %s%s_idx is null, n_%s = %d", who, name, name, cnt);
    for (int i = 0; i < cnt; ++i) {
        if (idx[i] < 0 || idx[i] >= len) return fail(PQ_ERR_INVALID, "dense KKT system batch: %s%s_idx[%d] = %d outside [0, %d)", who, name, i, idx[i], len);
        if (i > 0 && idx[i] <= idx[i - 1]) return fail(PQ_ERR_INVALID, "dense KKT system batch: %s%s_idx is not strictly ascending at %d", who, name, i);
    }
    return PQ_OK;
}

// the four lists of the batch (inst < 0) or of one instance: counts, order, range, and every row of G in h_l_idx or h_u_idx.  seen: m chars of scratch
int ksb_check_lists(int inst, int n, int m, const int cnt[4], const int* const lists[4], char* seen)
{
    static const char* const names[4] = {"h_l", "h_u", "x_l", "x_u"};
    char who[32] = "";
    if (inst >= 0) std::snprintf(who, sizeof(who), "instance %d: ", inst);
    for (int q = 0; q < 4; ++q)
        if (int rc = ksb_check_list(who, names[q], cnt[q], lists[q], q < 2 ? m : n)) return rc;
    std::memset(seen, 0, (size_t)m);
    for (int i = 0; i < cnt[0]; ++i) seen[lists[0][i]] = 1;
    for (int i = 0; i < cnt[1]; ++i) seen[lists[1][i]] = 1;
    for (int i = 0; i < m; ++i)
        if (!seen[i])
            return fail(PQ_ERR_INVALID, "dense KKT system batch: %srow %d of G is in neither h_l_idx nor h_u_idx (a row without a finite bound takes no part in a QP)", who, i);
    return PQ_OK;
}

// per-instance lists: counts [batch][4], the four list arrays [batch][m], [batch][m], [batch][n], [batch][n].  Every instance is checked, nothing is written
int ksb_check_all_lists(int batch, int n, int m, const int* counts, const int* h_l_idx, const int* h_u_idx, const int* x_l_idx, const int* x_u_idx, char* seen)
{
    if (!counts) return fail(PQ_ERR_INVALID, "dense KKT system batch: counts is null");
    for (int i = 0; i < batch; ++i) {
        const int* lists[4] = {h_l_idx ? h_l_idx + (size_t)i * m : nullptr, h_u_idx ? h_u_idx + (size_t)i * m : nullptr, x_l_idx ? x_l_idx + (size_t)i * n : nullptr,
                               x_u_idx ? x_u_idx + (size_t)i * n : nullptr};
        if (int rc = ksb_check_lists(i, n, m, counts + 4 * (size_t)i, lists, seen)) return rc;
    }
    return PQ_OK;
}

// checked per-instance lists into the host images of the tables (sized already) and the handle's summary counts
void ksb_take_lists(pq_kktsys_batch* k, const int* counts, const int* h_l_idx, const int* h_u_idx, const int* x_l_idx, const int* x_u_idx)
{
    const int n = k->n, m = k->m;
    const size_t stride = 2 * (size_t)m + 4 * (size_t)n;
    std::fill(k->tab_h.begin(), k->tab_h.end(), -1);
    std::copy(counts, counts + 4 * (size_t)k->batch, k->cnt_h.begin());
    for (int q = 0; q < 4; ++q) k->cnt[q] = 0;
    k->box_min[0] = k->box_min[1] = n;
    for (int i = 0; i < k->batch; ++i) {
        const int* c = counts + 4 * (size_t)i;
        int* t = k->tab_h.data() + i * stride;
        for (int e = 0; e < c[0]; ++e) t[h_l_idx[(size_t)i * m + e]] = e;
        for (int e = 0; e < c[1]; ++e) t[(size_t)m + h_u_idx[(size_t)i * m + e]] = e;
        for (int e = 0; e < c[2]; ++e) { const int j = x_l_idx[(size_t)i * n + e]; t[(size_t)2 * m + j] = e; t[(size_t)2 * m + 2 * n + e] = j; }
        for (int e = 0; e < c[3]; ++e) { const int j = x_u_idx[(size_t)i * n + e]; t[(size_t)2 * m + n + j] = e; t[(size_t)2 * m + 3 * n + e] = j; }
        for (int q = 0; q < 4; ++q) k->cnt[q] = std::max(k->cnt[q], c[q]);
        k->box_min[0] = std::min(k->box_min[0], c[2]);
        k->box_min[1] = std::min(k->box_min[1], c[3]);
    }
}

}  // namespace

// ---- the two heavy launches on their own, without the read-back of their success counts: what the public calls below do between their staging copies and their
// read-backs, and what the rounds of dense_solver_batch.hip launch with an activity word per instance.  Every pointer is device memory; the launch goes on the
// handle's stream and nothing waits for it.
namespace pq {

namespace {
// the kernel with or without a list, at one (KIND, G, PER)
template <int KIND, int G, bool PER>
void ksb_factor_go(bool sel, int grid, size_t lds, hipStream_t st, const KsbFactorArgs& a)
{
    if (sel) k_ksb_factor<KIND, G, PER, true><<<grid, DFB_THREADS, lds, st>>>(a);
    else k_ksb_factor<KIND, G, PER, false><<<grid, DFB_THREADS, lds, st>>>(a);
}
template <int KIND, bool PER>
void ksb_solve_go(bool sel, int grid, int threads, size_t lds, hipStream_t st, const KsbSolveArgs& a)
{
    if (sel) k_ksb_solve<KIND, PER, true><<<grid, threads, lds, st>>>(a);
    else k_ksb_solve<KIND, PER, false><<<grid, threads, lds, st>>>(a);
}
}  // namespace

void ksb_launch_factor(pq_kktsys_batch* k, const int* flags, const double* rho, const double* delta, const pq_vars& v, const int* active, const int* list, int count)
{
    pq_kkt_batch* kb = k->kb.get();
    const int n = k->n, batch = k->batch, slots = list ? count : batch;
    hipStream_t st = kb->st;
    KsbFactorArgs a;
    // (also for a launch masked by `active`: the one caller that masks, the solver's rounds, factors every instance in its first round.  A launch sized by a list
    // leaves the flag alone: instances outside the list may still wait with replaced lists and an old factor; the solver says when none does, ksb_lists_factored)
    if (!list) k->stale = false;
    a.n = n; a.p = k->p; a.m = k->m; a.ld = dfb_ld(n); a.width = n < 32 ? n : dfb_block_size_rule(n); a.count = slots; a.list = list; a.bd = ksb_bounds(k);
    a.Pu = kb->Pu.p; a.ATA = k->p > 0 ? kb->ATA.p : nullptr; a.GT = kb->GT.p;
    a.flags = flags; a.active = active; a.rho = rho; a.delta = delta;
    a.v_s_l = v.s_l; a.v_z_l = v.z_l; a.v_s_u = v.s_u; a.v_z_u = v.z_u; a.v_s_bl = v.s_bl; a.v_z_bl = v.z_bl; a.v_s_bu = v.s_bu; a.v_z_bu = v.z_bu;
    a.xbs = k->state[S_XBS].p; a.pdiag = k->state[S_PDIAG].p;
    a.reg_eps = k->settings.iterative_refinement_static_regularization_eps; a.reg_rel = k->settings.iterative_refinement_static_regularization_rel;
    a.s_l = k->state[S_SL].p; a.zinv_l = k->state[S_ZIL].p; a.s_u = k->state[S_SU].p; a.zinv_u = k->state[S_ZIU].p;
    a.s_bl = k->state[S_SBL].p; a.zinv_bl = k->state[S_ZIBL].p; a.s_bu = k->state[S_SBU].p; a.zinv_bu = k->state[S_ZIBU].p;
    a.z_reg = k->state[S_ZREG].p; a.rho_s = k->state[S_RHO].p; a.mdelta_s = k->state[S_MDELTA].p; a.use_ref = k->use_ref.p;
    a.delta_s = kb->delta_s.p; a.x_reg_s = kb->x_reg_s.p; a.zinv_s = kb->zinv_s.p; a.F = kb->fac.p; a.info = kb->status.p; a.badcol = kb->status.p + batch;
    const size_t lds = ksb_factor_lds_bytes(n);
    if (n < 32) {
        const int grid = div_up(slots, DFB_THREADS / 64);
        if (k->per_inst) {
            if (kb->kind == PQ_DENSE_CHOLESKY) ksb_factor_go<0, 64, true>(list != nullptr, grid, lds, st, a);
            else ksb_factor_go<1, 64, true>(list != nullptr, grid, lds, st, a);
        } else if (kb->kind == PQ_DENSE_CHOLESKY) ksb_factor_go<0, 64, false>(list != nullptr, grid, lds, st, a);
        else ksb_factor_go<1, 64, false>(list != nullptr, grid, lds, st, a);
    } else {
        if (k->per_inst) {
            if (kb->kind == PQ_DENSE_CHOLESKY) ksb_factor_go<0, DFB_THREADS, true>(list != nullptr, slots, lds, st, a);
            else ksb_factor_go<1, DFB_THREADS, true>(list != nullptr, slots, lds, st, a);
        } else if (kb->kind == PQ_DENSE_CHOLESKY) ksb_factor_go<0, DFB_THREADS, false>(list != nullptr, slots, lds, st, a);
        else ksb_factor_go<1, DFB_THREADS, false>(list != nullptr, slots, lds, st, a);
    }
    PQ_HIP(hipGetLastError());
}

void ksb_launch_solve(pq_kktsys_batch* k, const pq_vars& rhs, const pq_vars& lhs, const int* active, const int* list, int count)
{
    pq_kkt_batch* kb = k->kb.get();
    const int n = k->n, batch = k->batch, slots = list ? count : batch;
    hipStream_t st = kb->st;
    KsbSolveArgs a;
    a.n = n; a.p = k->p; a.m = k->m; a.ld = dfb_ld(n); a.bd = ksb_bounds(k); a.max_iter = k->settings.iterative_refinement_max_iter; a.batch = batch;
    a.eps_abs = k->settings.iterative_refinement_eps_abs; a.eps_rel = k->settings.iterative_refinement_eps_rel;
    a.min_rate = k->settings.iterative_refinement_min_improvement_rate;
    a.Pu = kb->Pu.p; a.AT = kb->AT.p; a.GT = kb->GT.p; a.F = kb->fac.p; a.delta_s = kb->delta_s.p; a.x_reg_s = kb->x_reg_s.p; a.zinv_s = kb->zinv_s.p; a.info = kb->status.p;
    a.active = active; a.list = list;
    a.s_l = k->state[S_SL].p; a.zinv_l = k->state[S_ZIL].p; a.s_u = k->state[S_SU].p; a.zinv_u = k->state[S_ZIU].p;
    a.s_bl = k->state[S_SBL].p; a.zinv_bl = k->state[S_ZIBL].p; a.s_bu = k->state[S_SBU].p; a.zinv_bu = k->state[S_ZIBU].p;
    a.z_reg = k->state[S_ZREG].p; a.mdelta_s = k->state[S_MDELTA].p; a.xbs = k->state[S_XBS].p;
    a.use_ref = k->use_ref.p;
    a.rhs = rhs; a.lhs = lhs;
    a.rhs_x_bar = k->state[S_RXB].p; a.rhs_z_bar = k->state[S_RZB].p; a.wy = k->wy.p; a.wz = k->wz.p; a.sinfo = k->sinfo.p; a.dinfo = k->dinfo.p;
    const int threads = n <= 64 ? 64 : KB_SOLVE_THREADS;
    const size_t lds = ksb_solve_lds_bytes(n);
    if (k->per_inst) {
        if (kb->kind == PQ_DENSE_CHOLESKY) ksb_solve_go<0, true>(list != nullptr, slots, threads, lds, st, a);
        else ksb_solve_go<1, true>(list != nullptr, slots, threads, lds, st, a);
    } else if (kb->kind == PQ_DENSE_CHOLESKY) ksb_solve_go<0, false>(list != nullptr, slots, threads, lds, st, a);
    else ksb_solve_go<1, false>(list != nullptr, slots, threads, lds, st, a);
    PQ_HIP(hipGetLastError());
}

void ksb_data_rewritten(pq_kktsys_batch* k, int options, bool refresh_ata, const double* x_b_scaling, const int* list, int count)
{
    if (options & PQ_KKT_UPDATE_P) ksb_extract_pdiag(k, list, count);
    if (refresh_ata) kb_refresh_ata(k->kb.get(), list, count);
    if (list) kb_scatter_rows(k->kb->st, k->state[S_XBS].p, x_b_scaling, list, (size_t)count, sizeof(double) * (size_t)k->n, true);
    else copy_in(k->state[S_XBS].p, x_b_scaling, k->state[S_XBS].bytes(), PQ_MEM_DEVICE, k->kb->st);
}

void ksb_lists_factored(pq_kktsys_batch* k) { k->stale = false; }
hipStream_t ksb_stream(pq_kktsys_batch* k) { return k->kb->st; }
const int* ksb_factor_status(const pq_kktsys_batch* k) { return k->kb->status.p; }
const int* ksb_solve_info(const pq_kktsys_batch* k) { return k->sinfo.p; }

// after launches of the two functions above: the host side of both handles as the public calls leave it (status, counts and diagnostics read back; waits)
void ksb_refresh_host(pq_kktsys_batch* k)
{
    const int batch = k->batch;
    const KbReadback more[2] = {{k->sinfo_h.p, k->sinfo.p, sizeof(int) * 3 * batch}, {k->dinfo_h.p, k->dinfo.p, sizeof(double) * 2 * batch}};
    kb_factor_done(k->kb.get(), nullptr, more, 2);  // (the rounds' launches are not timed by the backend's events)
    int solved = 0;
    for (int b = 0; b < batch; ++b) solved += k->sinfo_h.p[b] != 0;
    k->n_solved = solved; k->solved = true;
}

// instance j of the new handle is instance sel.host[j] of k, over a backend cloned by the same list.  Gathered: every state vector (P_diag and x_b_scaling
// included), use_ref, the diagnostics of the last solve -- sinfo is three arrays of [batch] in one buffer and dinfo two, on the device and in their pinned images, one
// gather each -- and with lists per instance the rows of tab (2 m + 4 n ints) and cnt_d with their host images, from which the summary counts are taken again.  Shared
// lists: the one table is copied.  The work vectors, the refinement flags' staging, the host-mode staging and the events are only sized.
pq_kktsys_batch* ksb_clone_rows(const pq_kktsys_batch* k, const KbSelect& sel)
{
    std::unique_ptr<pq_kkt_batch, KbDeleter> own(kb_clone_rows(k->kb.get(), sel));
    PQ_HIP(hipSetDevice(k->device));
    stream_wait(k->kb->st);
    std::unique_ptr<pq_kktsys_batch> c(new pq_kktsys_batch);
    const int count = sel.count;
    const size_t b = (size_t)count, sb = (size_t)k->batch, stride = 2 * (size_t)k->m + 4 * (size_t)k->n;
    c->device = k->device; c->batch = count; c->n = k->n; c->p = k->p; c->m = k->m;
    c->settings = k->settings;
    c->per_inst = k->per_inst; c->stale = k->stale; c->solved = k->solved; c->seen = k->seen;
    if (k->per_inst) {
        c->tab_h.resize(b * stride); c->cnt_h.resize(4 * b);
        kb_gather_host(c->tab_h.data(), k->tab_h.data(), sel.host, count, stride);
        kb_gather_host(c->cnt_h.data(), k->cnt_h.data(), sel.host, count, 4);
        c->box_min[0] = c->box_min[1] = k->n;
        for (int j = 0; j < count; ++j) {
            const int* cj = c->cnt_h.data() + 4 * (size_t)j;
            for (int q = 0; q < 4; ++q) c->cnt[q] = std::max(c->cnt[q], cj[q]);
            c->box_min[0] = std::min(c->box_min[0], cj[2]);
            c->box_min[1] = std::min(c->box_min[1], cj[3]);
        }
    } else {
        for (int q = 0; q < 4; ++q) { c->cnt[q] = k->cnt[q]; c->idx[q] = k->idx[q]; }
        c->box_min[0] = k->box_min[0]; c->box_min[1] = k->box_min[1];
    }
    c->kb = std::move(own);
    ksb_alloc(c.get());
    hipStream_t st = c->kb->st;
    PQ_HIP(hipEventRecord(c->ev[0], st));
    if (k->per_inst) {
        kb_gather_rows(st, c->tab.p, k->tab.p, sel.dev, b, sizeof(int) * stride);
        kb_gather_rows(st, c->cnt_d.p, k->cnt_d.p, sel.dev, b, sizeof(int) * 4);
    } else if (k->tab.n) PQ_HIP(hipMemcpyAsync(c->tab.p, k->tab.p, k->tab.bytes(), hipMemcpyDeviceToDevice, st));
    for (int s = 0; s < S_COUNT; ++s)
        if (k->state[s].n) kb_gather_rows(st, c->state[s].p, k->state[s].p, sel.dev, b, sizeof(double) * ksb_state_len(k, s));
    kb_gather_rows(st, c->use_ref.p, k->use_ref.p, sel.dev, b, sizeof(int));
    for (int h = 0; h < 3; ++h) {
        kb_gather_rows(st, c->sinfo.p + h * b, k->sinfo.p + h * sb, sel.dev, b, sizeof(int));
        kb_gather_host(c->sinfo_h.p + h * b, k->sinfo_h.p + h * sb, sel.host, count, 1);
    }
    for (int h = 0; h < 2; ++h) {
        kb_gather_rows(st, c->dinfo.p + h * b, k->dinfo.p + h * sb, sel.dev, b, sizeof(double));
        kb_gather_host(c->dinfo_h.p + h * b, k->dinfo_h.p + h * sb, sel.host, count, 1);
    }
    for (int j = 0; j < count && k->solved; ++j) c->n_solved += c->sinfo_h.p[j] != 0;
    PQ_HIP(hipEventRecord(c->ev[1], st));
    kb_gather_timed(sel, st, c->ev[0], c->ev[1]);
    return c.release();
}

}  // namespace pq

extern "C" {

// what the two creators share once the lists are checked: the backend, the allocations, the tables, x_b_scaling and P_diag.  counts / lists: the four counts and lists
// of the batch, or with per_inst [batch][4] and four arrays of `batch` rows
static int ksb_create(pq_kktsys_batch** out, int device, int batch, int n, int p, int m, const double* P_utri, const double* AT, const double* GT, bool per_inst,
                      const int* counts, const int* const lists[4], const double* x_b_scaling, const pq_settings* settings, int mem)
{
    // (the backend's create checks its arguments before it touches the device, too)
    pq_kkt_batch* kb = nullptr;
    if (int rc = pq_kkt_batch_create_dense(&kb, device, batch, n, p, m, settings->kkt_solver, P_utri, AT, GT, mem)) return rc;
    std::unique_ptr<pq_kkt_batch, KbDeleter> own(kb);
    return guarded([&] {
        PQ_HIP(hipSetDevice(device));
        std::unique_ptr<pq_kktsys_batch> k(new pq_kktsys_batch);
        k->device = device; k->batch = batch; k->n = n; k->p = p; k->m = m;
        k->settings = *settings;
        k->per_inst = per_inst;
        k->seen.assign((size_t)m, 0);
        if (per_inst) {
            k->tab_h.assign((size_t)batch * (2 * (size_t)m + 4 * (size_t)n), -1);
            k->cnt_h.assign(4 * (size_t)batch, 0);
            ksb_take_lists(k.get(), counts, lists[0], lists[1], lists[2], lists[3]);
        } else {
            for (int q = 0; q < 4; ++q) { k->cnt[q] = counts[q]; k->idx[q].assign(lists[q], lists[q] + counts[q]); }
            k->box_min[0] = counts[2]; k->box_min[1] = counts[3];
        }
        k->kb = std::move(own);
        ksb_alloc(k.get());
        ksb_upload_tables(k.get());
        hipStream_t st = k->kb->st;
        if (x_b_scaling) copy_in(k->state[S_XBS].p, x_b_scaling, k->state[S_XBS].bytes(), mem, st);
        else {
            const std::vector<double> ones((size_t)batch * n, 1.0);
            PQ_HIP(hipMemcpyAsync(k->state[S_XBS].p, ones.data(), sizeof(double) * ones.size(), hipMemcpyHostToDevice, st));
            stream_wait(st);
        }
        ksb_extract_pdiag(k.get());
        stream_wait(st);
        *out = k.release();
        return (int)PQ_OK;
    });
}

static int ksb_check_create(pq_kktsys_batch** out, int batch, int n, int p, int m, const pq_settings* settings)
{
    if (!out) return fail(PQ_ERR_INVALID, "null argument");
    if (batch < 1 || n < 1 || p < 0 || m < 0)
        return fail(PQ_ERR_INVALID, "dense KKT system batch: batch = %d, n = %d, p = %d, m = %d: batch, n >= 1 and p, m >= 0 wanted", batch, n, p, m);
    return ksb_check_settings(settings);
}

int pq_kktsys_batch_create_dense(pq_kktsys_batch** out, int device, int batch, int n, int p, int m, const double* P_utri, const double* AT, const double* GT, int n_h_l,
                                 int n_h_u, int n_x_l, int n_x_u, const int* h_l_idx, const int* h_u_idx, const int* x_l_idx, const int* x_u_idx, const double* x_b_scaling,
                                 const pq_settings* settings, int mem)
{
    if (int rc = ksb_check_create(out, batch, n, p, m, settings)) return rc;
    const int cnt[4] = {n_h_l, n_h_u, n_x_l, n_x_u};
    const int* lists[4] = {h_l_idx, h_u_idx, x_l_idx, x_u_idx};
    std::vector<char> seen((size_t)m, 0);
    if (int rc = ksb_check_lists(-1, n, m, cnt, lists, seen.data())) return rc;
    return ksb_create(out, device, batch, n, p, m, P_utri, AT, GT, false, cnt, lists, x_b_scaling, settings, mem);
}

int pq_kktsys_batch_create_dense_lists(pq_kktsys_batch** out, int device, int batch, int n, int p, int m, const double* P_utri, const double* AT, const double* GT,
                                       const int* counts, const int* h_l_idx, const int* h_u_idx, const int* x_l_idx, const int* x_u_idx, const double* x_b_scaling,
                                       const pq_settings* settings, int mem)
{
    if (int rc = ksb_check_create(out, batch, n, p, m, settings)) return rc;
    std::vector<char> seen((size_t)m, 0);
    if (int rc = ksb_check_all_lists(batch, n, m, counts, h_l_idx, h_u_idx, x_l_idx, x_u_idx, seen.data())) return rc;
    const int* lists[4] = {h_l_idx, h_u_idx, x_l_idx, x_u_idx};
    return ksb_create(out, device, batch, n, p, m, P_utri, AT, GT, true, counts, lists, x_b_scaling, settings, mem);
}

int pq_kktsys_batch_set_lists(pq_kktsys_batch* k, const int* counts, const int* h_l_idx, const int* h_u_idx, const int* x_l_idx, const int* x_u_idx)
{
    if (!k) return fail(PQ_ERR_INVALID, "null argument");
    if (!k->per_inst) return fail(PQ_ERR_INVALID, "dense KKT system batch: set_lists: the handle's lists are shared by the batch (pq_kktsys_batch_create_dense_lists makes the other kind)");
    if (int rc = ksb_check_all_lists(k->batch, k->n, k->m, counts, h_l_idx, h_u_idx, x_l_idx, x_u_idx, k->seen.data())) return rc;
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        stream_wait(k->kb->st);  // (a launch that still reads the tables; the host images are pageable)
        ksb_take_lists(k, counts, h_l_idx, h_u_idx, x_l_idx, x_u_idx);
        ksb_upload_tables(k);
        k->stale = true;  // the factors and the stored scalings belong to the old lists
        k->solved = false;
        return (int)PQ_OK;
    });
}

void pq_kktsys_batch_destroy(pq_kktsys_batch* k) { delete k; }

int pq_kktsys_batch_clone(const pq_kktsys_batch* k, pq_kktsys_batch** out)
{
    if (!k || !out) return fail(PQ_ERR_INVALID, "null argument");
    pq_kkt_batch* kb = nullptr;
    if (int rc = pq_kkt_batch_clone(k->kb.get(), &kb)) return rc;
    std::unique_ptr<pq_kkt_batch, KbDeleter> own(kb);
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        stream_wait(k->kb->st);
        std::unique_ptr<pq_kktsys_batch> c(new pq_kktsys_batch);
        c->device = k->device; c->batch = k->batch; c->n = k->n; c->p = k->p; c->m = k->m;
        c->settings = k->settings;
        for (int q = 0; q < 4; ++q) { c->cnt[q] = k->cnt[q]; c->idx[q] = k->idx[q]; }
        c->per_inst = k->per_inst; c->stale = k->stale; c->box_min[0] = k->box_min[0]; c->box_min[1] = k->box_min[1];
        c->tab_h = k->tab_h; c->cnt_h = k->cnt_h; c->seen = k->seen;
        c->n_solved = k->n_solved; c->solved = k->solved;
        c->kb = std::move(own);
        ksb_alloc(c.get());
        ksb_upload_tables(c.get());
        hipStream_t st = c->kb->st;
        for (int s = 0; s < S_COUNT; ++s)
            if (k->state[s].n) PQ_HIP(hipMemcpyAsync(c->state[s].p, k->state[s].p, k->state[s].bytes(), hipMemcpyDeviceToDevice, st));
        PQ_HIP(hipMemcpyAsync(c->use_ref.p, k->use_ref.p, k->use_ref.bytes(), hipMemcpyDeviceToDevice, st));
        std::memcpy(c->sinfo_h.p, k->sinfo_h.p, sizeof(int) * 3 * (size_t)k->batch);
        std::memcpy(c->dinfo_h.p, k->dinfo_h.p, sizeof(double) * 2 * (size_t)k->batch);
        stream_wait(st);
        *out = c.release();
        return (int)PQ_OK;
    });
}

int pq_kktsys_batch_clone_select(const pq_kktsys_batch* k, const int* idx, int count, pq_kktsys_batch** out)
{
    if (!k || !out) return fail(PQ_ERR_INVALID, "null argument");
    if (int rc = kb_check_select("dense KKT system batch", k->batch, idx, count)) return rc;
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        DBuf<int> idx_d((size_t)count);
        PQ_HIP(hipMemcpy(idx_d.p, idx, sizeof(int) * (size_t)count, hipMemcpyHostToDevice));
        *out = ksb_clone_rows(k, KbSelect{idx, idx_d.p, count, nullptr});
        return (int)PQ_OK;
    });
}

int pq_kktsys_batch_dims(const pq_kktsys_batch* k, int* batch, int* n, int* p, int* m)
{
    if (!k) return fail(PQ_ERR_INVALID, "null argument");
    if (batch) *batch = k->batch;
    if (n) *n = k->n;
    if (p) *p = k->p;
    if (m) *m = k->m;
    return PQ_OK;
}

pq_kkt_batch* pq_kktsys_batch_backend(pq_kktsys_batch* k)
{
    if (!k) { fail(PQ_ERR_INVALID, "null argument"); return nullptr; }
    return k->kb.get();
}

int pq_kktsys_batch_update_data_dense(pq_kktsys_batch* k, const double* P_utri, const double* AT, const double* GT, const double* x_b_scaling, int options, int mem)
{
    if (!k) return fail(PQ_ERR_INVALID, "null argument");
    if (int rc = pq_kkt_batch_update_data_dense(k->kb.get(), P_utri, AT, GT, options, mem)) return rc;
    if (!x_b_scaling && !(options & PQ_KKT_UPDATE_P)) return PQ_OK;
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        if (options & PQ_KKT_UPDATE_P) ksb_extract_pdiag(k);
        if (x_b_scaling) copy_in(k->state[S_XBS].p, x_b_scaling, k->state[S_XBS].bytes(), mem, k->kb->st);
        stream_wait(k->kb->st);
        return (int)PQ_OK;
    });
}

int pq_kktsys_batch_set_settings(pq_kktsys_batch* k, const pq_settings* settings)
{
    if (!k) return fail(PQ_ERR_INVALID, "null argument");
    if (int rc = ksb_check_settings(settings)) return rc;
    const int kind = k->settings.kkt_solver;
    k->settings = *settings;
    k->settings.kkt_solver = kind;
    return PQ_OK;
}

int pq_kktsys_batch_update_scalings_and_factor(pq_kktsys_batch* k, const int* iterative_refinement, const double* rho, const double* delta, const pq_vars* vars, int mem)
{
    if (!k || !rho || !delta || !vars) return fail(PQ_ERR_INVALID, "null argument");
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense KKT system batch: bad mem");
    if (int rc = ksb_check_vars(k, vars, 2, "update_scalings_and_factor")) return rc;
    int good = 0;
    const int rc = guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        pq_kkt_batch* kb = k->kb.get();
        const int batch = k->batch;
        const auto w0 = std::chrono::steady_clock::now();
        hipStream_t st = kb->st;
        size_t off = 0, foff = 0;
        const int* flags = iterative_refinement ? kb_in(k->flags_d, st, iterative_refinement, (size_t)batch, mem, foff) : nullptr;
        const double* rho_d = kb_in(k->stage_in, st, rho, (size_t)batch, mem, off);
        const double* delta_d = kb_in(k->stage_in, st, delta, (size_t)batch, mem, off);
        const pq_vars v = ksb_vars_in(k, vars, 2, mem, off);
        PQ_HIP(hipEventRecord(kb->ev[0], st));
        ksb_launch_factor(k, flags, rho_d, delta_d, v, nullptr, nullptr, k->batch);
        PQ_HIP(hipEventRecord(kb->ev[1], st));
        good = kb_factor_done(kb, &w0);  // the backend handle: as its own update_scalings_and_factor leaves it
        return (int)PQ_OK;
    });
    return rc == PQ_OK ? good : rc;
}

int pq_kktsys_batch_solve(pq_kktsys_batch* k, const pq_vars* rhs, pq_vars* lhs, int mem)
{
    if (!k || !rhs || !lhs) return fail(PQ_ERR_INVALID, "null argument");
    if (!k->kb->computed || k->stale) return fail(PQ_ERR_INVALID, "dense KKT system batch: solve before update_scalings_and_factor");
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense KKT system batch: bad mem");
    if (int rc = ksb_check_vars(k, rhs, 0, "solve: rhs")) return rc;
    if (int rc = ksb_check_vars(k, lhs, 0, "solve: lhs")) return rc;
    if (int rc = ksb_check_settings(&k->settings)) return rc;
    int good = 0;
    const int rc = guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        pq_kkt_batch* kb = k->kb.get();
        const int batch = k->batch;
        hipStream_t st = kb->st;
        size_t off = 0;
        const pq_vars r = ksb_vars_in(k, rhs, 0, mem, off);
        const pq_vars l = ksb_vars_out(k, lhs, mem, kb->n_ok < batch);
        PQ_HIP(hipEventRecord(k->ev[0], st));
        ksb_launch_solve(k, r, l, nullptr, nullptr, k->batch);
        PQ_HIP(hipEventRecord(k->ev[1], st));
        ksb_vars_back(k, lhs, l, mem);
        PQ_HIP(hipMemcpyAsync(k->sinfo_h.p, k->sinfo.p, sizeof(int) * 3 * batch, hipMemcpyDeviceToHost, st));
        PQ_HIP(hipMemcpyAsync(k->dinfo_h.p, k->dinfo.p, sizeof(double) * 2 * batch, hipMemcpyDeviceToHost, st));
        stream_wait(st);
        for (int b = 0; b < batch; ++b) good += k->sinfo_h.p[b] != 0;
        k->n_solved = good;
        k->solved = true;
        k->timed[0] = true;
        return (int)PQ_OK;
    });
    return rc == PQ_OK ? good : rc;
}

int pq_kktsys_batch_mul(pq_kktsys_batch* k, const pq_vars* lhs, pq_vars* rhs, int mem)
{
    if (!k || !lhs || !rhs) return fail(PQ_ERR_INVALID, "null argument");
    if (!k->kb->computed || k->stale) return fail(PQ_ERR_INVALID, "dense KKT system batch: mul before update_scalings_and_factor");
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense KKT system batch: bad mem");
    if (int rc = ksb_check_vars(k, lhs, 0, "mul: lhs")) return rc;
    if (int rc = ksb_check_vars(k, rhs, 0, "mul: rhs")) return rc;
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        pq_kkt_batch* kb = k->kb.get();
        hipStream_t st = kb->st;
        size_t off = 0;
        KsbMulArgs a;
        a.n = k->n; a.p = k->p; a.m = k->m; a.bd = ksb_bounds(k);
        a.Pu = kb->Pu.p; a.AT = kb->AT.p; a.GT = kb->GT.p;
        a.s_l = k->state[S_SL].p; a.zinv_l = k->state[S_ZIL].p; a.s_u = k->state[S_SU].p; a.zinv_u = k->state[S_ZIU].p;
        a.s_bl = k->state[S_SBL].p; a.zinv_bl = k->state[S_ZIBL].p; a.s_bu = k->state[S_SBU].p; a.zinv_bu = k->state[S_ZIBU].p;
        a.rho_s = k->state[S_RHO].p; a.mdelta_s = k->state[S_MDELTA].p; a.xbs = k->state[S_XBS].p;
        a.lhs = ksb_vars_in(k, lhs, 0, mem, off);
        a.rhs = ksb_vars_out(k, rhs, mem, false);
        a.wz = k->wz.p;
        PQ_HIP(hipEventRecord(k->ev[2], st));
        if (k->per_inst) k_ksb_mul<true><<<k->batch, KB_SOLVE_THREADS, 0, st>>>(a);
        else k_ksb_mul<false><<<k->batch, KB_SOLVE_THREADS, 0, st>>>(a);
        PQ_HIP(hipGetLastError());
        PQ_HIP(hipEventRecord(k->ev[3], st));
        ksb_vars_back(k, rhs, a.rhs, mem);
        stream_wait(st);
        k->timed[1] = true;
        return (int)PQ_OK;
    });
}

int pq_kktsys_batch_info(const pq_kktsys_batch* k, int* solve_ok, int* refine_steps, int* backend_solves, double* refine_error, double* rhs_norm)
{
    if (!k) return fail(PQ_ERR_INVALID, "null argument");
    if (!k->solved) return fail(PQ_ERR_INVALID, "dense KKT system batch: no solve yet");
    const size_t b = (size_t)k->batch;
    for (size_t i = 0; i < b; ++i) {
        if (solve_ok) solve_ok[i] = k->sinfo_h.p[i];
        if (refine_steps) refine_steps[i] = k->sinfo_h.p[b + i];
        if (backend_solves) backend_solves[i] = k->sinfo_h.p[2 * b + i];
        if (refine_error) refine_error[i] = k->dinfo_h.p[i];
        if (rhs_norm) rhs_norm[i] = k->dinfo_h.p[b + i];
    }
    return PQ_OK;
}

int pq_kktsys_batch_state(pq_kktsys_batch* k, int what, double* out_host)
{
    if (!k || !out_host) return fail(PQ_ERR_INVALID, "null argument");
    if (what < PQ_KKTSYS_BATCH_X_REG || what > PQ_KKTSYS_BATCH_RHS_Z_BAR) return fail(PQ_ERR_INVALID, "dense KKT system batch: state %d: 0 .. 3 wanted", what);
    if (!k->kb->computed || k->stale) return fail(PQ_ERR_INVALID, "dense KKT system batch: no factorisation yet");
    if (what >= PQ_KKTSYS_BATCH_RHS_X_BAR && !k->solved) return fail(PQ_ERR_INVALID, "dense KKT system batch: no solve yet");
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        const DBuf<double>& src = what == PQ_KKTSYS_BATCH_X_REG ? k->kb->x_reg_s : what == PQ_KKTSYS_BATCH_Z_REG ? k->state[S_ZREG] : what == PQ_KKTSYS_BATCH_RHS_X_BAR ? k->state[S_RXB] : k->state[S_RZB];
        if (src.n) PQ_HIP(hipMemcpyAsync(out_host, src.p, src.bytes(), hipMemcpyDeviceToHost, k->kb->st));
        stream_wait(k->kb->st);
        return (int)PQ_OK;
    });
}

int pq_kktsys_batch_last_ms(const pq_kktsys_batch* k, double out3[3])
{
    if (!k || !out3) return fail(PQ_ERR_INVALID, "null argument");
    return guarded([&] {
        PQ_HIP(hipSetDevice(k->device));
        float ms = 0.f;
        if (k->kb->timed[0]) PQ_HIP(hipEventElapsedTime(&ms, k->kb->ev[0], k->kb->ev[1]));
        out3[0] = ms;
        for (int s = 0; s < 2; ++s) {
            ms = 0.f;
            if (k->timed[s]) PQ_HIP(hipEventElapsedTime(&ms, k->ev[2 * s], k->ev[2 * s + 1]));
            out3[1 + s] = ms;
        }
        return (int)PQ_OK;
    });
}

}  // extern "C"
