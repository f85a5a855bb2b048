// piqp_amd/csrc/dense_solver_batch.hip -- pq_solver_batch_*: piqp::DenseSolver::setup() / solve() (solver.hpp:69-216, 379-1259) for a BATCH of small dense QPs
// (n <= 128) over the batched KKTSystem (dense_kktsys_batch.hip).  Per instance every number is the CPU oracle's (oracle/orc_solver.c) bit for bit.  This file is
// compiled with -ffp-contract=off (piqp_amd/build.py, NO_CONTRACT) like orc_solver.c: every product and every sum is rounded on its own; the three mat-vec evaluators
// inside update_residuals_nr are the contracted orc_dense.c and are written with explicit fma(): kb_eval_P_row, kb_gemv_t_col, kb_gemv_n_row of
// dense_kkt_batch_device.hpp.
//
// The solve runs in ROUNDS clocked by the host.  The interior-point state of every instance (result, res_nr, res, step, prox, the pq_info fields, the refinement
// flag and a stage word) lives in device memory.  orc_solver.c:664-953 is cut at its calls into KKTSystem:
//
//   stage (where the instance resumes)    k_dsb_advance does                                                         and asks for
//   INIT      :675-690                    resets info, s = z = 1 on the bounded rows                                 FACTOR
//   FACTOR0   :693-709                    failed: the retry ladder (refinement on, then x 100, reg_limit) or NUMERICS FACTOR / DONE
//                                         else the right-hand side (-c, b, -h_l, h_u, -x_l, x_u, 0)                  SOLVE
//   SOLVE0    :712-761, then the loop     step -> result (a copy of bits), the shift, mu, the prox copies            (loop head)
//   FACTOR    :828-851 / :926             the ladder of :828-838; else update_residuals_r if the regularisation      SOLVE
//                                         changed, the predictor right-hand side
//   PRED      :854-879                    calculate_step, sigma, the corrector right-hand side                       SOLVE
//   CORR      :882-924, then the loop     the step, mu, update_residuals_nr, the rho / delta and prox updates        (loop head)
//   NOINEQ    :929-948, then the loop     the same without inequalities
//   loop head :763-824                    MAX_ITER_REACHED, update_residuals_nr at iteration 0, the trace row, the   FACTOR / DONE
//                                         three exits, update_residuals_r, the boundary shift, the fine-tuning
//
// A round is: k_dsb_advance (one workgroup per instance: from its stage to its next KKTSystem call or its end; it writes rho, delta and the flag for a factorisation,
// the right-hand side into `res` for a solve, an activity word for each of the two launches and adds itself to one of three counters), the counters read back through
// pinned memory, then the factor launch k_ksb_factor and the solve launch k_ksb_solve of dense_kktsys_batch.hip, each masked by its activity words and skipped when its
// counter is zero.  Every solve writes into `step`; the very first one of the reference writes into `result`, so SOLVE0 copies.  The loop ends when DONE == batch; the
// number of rounds is bounded before it starts ((max_iter + 1) (max_factor_retires + 4)), a loop that reaches the bound returns PQ_ERR_INTERNAL.  No kernel here polls
// memory, waits for another workgroup or loops on a condition computed from floating-point data (the Ruiz loop is counted, with the oracle's early exit).
//
// update() (solver.hpp:218-308, orc_solver.c:357-384) runs where the data stand, on the backend's own Pu, AT, GT and the vectors here: k_dsb_unscale, the assignment
// (k_dsb_ingest for a given matrix, copies for c and b, the bound vectors through the host logic of the lists), then k_dsb_ruiz -- with the stored scalings when
// preconditioner_reuse_on_update is set or no matrix was given, else the equilibration from delta = 1 on the unscaled data.  Unscaling and rescaling do not give the
// stored bits back: an update of c alone moves P, A' and G' by roundings, and the kernels run the oracle's multiplications in the oracle's order.  With shared bound
// sets (the default) the finite-bound set stays the setup's (it is baked into the KKT system and into `tab`); a call whose lists would differ is refused before
// anything is written.  With PQ_BOUND_SETS_PER_INSTANCE (pq_solver_batch_set_bound_sets) every instance has lists of its own: `tab` has a row and `cnt_d` four counts
// per instance (KbBounds; the kernels below are built twice, PER = false being the code of before, PER = true taking row and counts from the instance), and an update replaces the lists -- the unscaling still runs
// on the old tables, everything after it on the new ones -- here and in the KKT system (pq_kktsys_batch_set_lists).  The host logic of the lists is ONE function for
// both modes, setup and update: dsb_bound_lists.
// ONE RULE IS NOT THE REFERENCE'S.  dense/kkt.hpp:62-71 (orc_dense.c:609-613) recomputes A'A only when A is given.  When P or G comes without A and the scalings are
// recomputed, A' is rescaled with the new scalings and A'A stays that of the old ones: on the oracle this turns solvable problems into MAX_ITER_REACHED or
// PRIMAL_INFEASIBLE.  Here A'A is recomputed from the rescaled A' when A is given, or when any matrix is given and preconditioner_reuse_on_update == 0; in every other
// case (vectors only; matrices without A under reuse) it is left alone as the reference leaves it, where the staleness is rounding only.  The single dense backends
// refresh A'A at every update for the same reason (dense_exact.hip, dense_kkt.cpp).  The oracle reaches the same state with update(..., A = its own unscaled A).
//
// Arithmetic: every dot product and every sigma sum is ONE sequential chain in index order, each chain on a lane of its own (the lanes pick their operands, then run
// the same loop); maxima and minima are order-independent and are wave / workgroup reductions (the maximum of :581-615 is SIGNED; inf_scaled is NaN-sticky).  The
// scalar logic runs on lane 0 on the instance's state in LDS.
// Memory: the vectors a launch writes and reads again are reached through plain pointers only (dense_kkt_batch_device.hpp says why), with __syncthreads() between
// the phases.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <vector>

#include "dense_kkt_batch_internal.hpp"

namespace pq {

namespace {

constexpr int DSB_T = 128;       // threads of k_dsb_advance, k_dsb_finish
constexpr int DSB_RUIZ_T = 256;  // threads of k_dsb_ruiz, k_dsb_unscale
constexpr double DSB_INF = 1e30;  // fwd.hpp:54 PIQP_INF

enum { ST_INIT = 0, ST_FACTOR0, ST_SOLVE0, ST_FACTOR, ST_PRED, ST_CORR, ST_NOINEQ, ST_DONE };
enum { WANT_FACTOR = 0, WANT_SOLVE = 1, WANT_DONE = 2 };

// one instance's scalar state (device memory; in LDS while k_dsb_advance runs)
struct DsbState {
    pq_info info;
    int stage, enable_ref, reg_changed, trace_rows;
};
static_assert(sizeof(DsbState) % sizeof(int) == 0, "copied as ints");

struct DsbVars {
    double *x, *y, *z_l, *z_u, *z_bl, *z_bu, *s_l, *s_u, *s_bl, *s_bu;
};
__host__ __device__ inline DsbVars dsb_at(const pq_vars& v, size_t on, size_t op, size_t om)
{
    return DsbVars{v.x + on, v.y + op, v.z_l + om, v.z_u + om, v.z_bl + on, v.z_bu + on, v.s_l + om, v.s_u + om, v.s_bl + on, v.s_bu + on};
}

__device__ __forceinline__ double dsb_dmax(double a, double b) { return a > b ? a : b; }  // orc_solver.c:31-32
__device__ __forceinline__ double dsb_dmin(double a, double b) { return a < b ? a : b; }

// ---- reductions over the workgroup: K values at once; every thread gets the results
enum { R_MAX = 0, R_MAXNAN = 1, R_MIN = 2 };
__device__ __forceinline__ double dsb_comb(double a, double o, int op)
{
    if (op == R_MAXNAN) return (a != a || o != o) ? __builtin_nan("") : (a > o ? a : o);
    if (op == R_MAX) return o > a ? o : a;
    return o < a ? o : a;
}
template <int K>
__device__ __forceinline__ void dsb_reduce(double (&v)[K], const int (&op)[K], double* red)
{
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] = dsb_comb(v[k], __shfl_xor(v[k], off, 64), op[k]);
    const int waves = blockDim.x >> 6;
    __syncthreads();  // (the results before have been read)
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double r = red[k];
        for (int w = 1; w < waves; ++w) r = dsb_comb(r, red[w * K + k], op[k]);
        v[k] = r;
    }
}
constexpr int DSB_RED = 8 * (DSB_RUIZ_T / 64);  // doubles of `red`

// ---- the sequential chains (orc_solver.c:439)
__device__ __forceinline__ double dsb_dot(const double* a, const double* b, int len)
{
    double s = 0.0;
    for (int i = 0; i < len; ++i) s = s + a[i] * b[i];
    return s;
}

// ---- the interior-point state machine
struct DsbArgs {
    int n, p, m, batch, trace_max, slot;
    KbBounds bd;                                          // the finite-bound tables: of the batch, or one row and four counts per instance
    pq_settings set;
    const double *Pu, *AT, *GT;                           // the backend's (scaled) data
    const double *c, *b, *h_l, *h_u, *x_l, *x_u, *xbs;    // scaled, [batch][len]
    const double *pd, *pdb, *pdi, *pdbi, *pc_inv;         // the preconditioner: delta [n + p + m], delta_b [n], their inverses, 1 / c
    pq_vars r, nr, res, st, px;                           // result, res_nr, res, step, prox
    DsbState* state;
    double *rho, *delta;                                  // [batch]: what the factor launch reads
    int *flags, *act_f, *act_s, *counters;                // counters: [2][4], the slot of this round and the one zeroed for the next
    const int *fstatus, *sinfo;                           // the factor launch's status, the solve launch's diagnostics
    double* trace;                                        // [batch][trace_max][11]
    const int* list;                                      // SEL only: one workgroup per entry, workgroup s is instance list[s] (distinct entries).  Every array above,
                                                          // the activity words and the state included, is indexed by INSTANCE
};

// what one instance's workgroup keeps at hand
struct DsbCtx {
    int n, p, m, nxl, nxu, t;
    double cnt, ci;
    const double *Pu, *AT, *GT, *c, *b, *h_l, *h_u, *x_l, *x_u, *xbs, *pd, *pdb, *pdi, *pdbi;
    const int *has_l, *has_u, *xl_idx, *xu_idx;
    DsbVars r, nr, res, st, px;
    DsbState* S;  // LDS
    double *sc, *red;  // LDS: 16 scalars, the reductions' scratch
};

// calculate_mu :443-448; every thread gets it
__device__ __forceinline__ double dsb_mu(const DsbCtx& C)
{
    __syncthreads();
    const int t = C.t;
    const double* a = t == 0 ? C.r.s_l : t == 1 ? C.r.s_u : t == 2 ? C.r.s_bl : C.r.s_bu;
    const double* b = t == 0 ? C.r.z_l : t == 1 ? C.r.z_u : t == 2 ? C.r.z_bl : C.r.z_bu;
    const int len = t < 2 ? C.m : t == 2 ? C.nxl : t == 3 ? C.nxu : 0;
    const double s = dsb_dot(a, b, len);
    if (t < 4) C.sc[8 + t] = s;
    __syncthreads();
    return (C.sc[8] + C.sc[9] + C.sc[10] + C.sc[11]) / C.cnt;
}

// primal_res_of and dual_res_of :484-494 of one set of variables
__device__ __forceinline__ void dsb_res_norms(const DsbCtx& C, const DsbVars& v, double& primal, double& dual)
{
    const int n = C.n, p = C.p, m = C.m, t = C.t;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = t; j < p; j += DSB_T) a[0] = dsb_comb(a[0], fabs(v.y[j] * 1.0 * C.pdi[n + j]), R_MAXNAN);
    for (int j = t; j < m; j += DSB_T) {
        a[1] = dsb_comb(a[1], fabs(v.z_l[j] * 1.0 * C.pdi[n + p + j]), R_MAXNAN);
        a[2] = dsb_comb(a[2], fabs(v.z_u[j] * 1.0 * C.pdi[n + p + j]), R_MAXNAN);
    }
    for (int i = t; i < C.nxl; i += DSB_T) a[3] = dsb_comb(a[3], v.z_bl[i] * C.pdbi[C.xl_idx[i]], R_MAX);
    for (int i = t; i < C.nxu; i += DSB_T) a[3] = dsb_comb(a[3], v.z_bu[i] * C.pdbi[C.xu_idx[i]], R_MAX);
    for (int i = t; i < n; i += DSB_T) a[4] = dsb_comb(a[4], fabs(v.x[i] * C.ci * C.pdi[i]), R_MAXNAN);
    const int op[5] = {R_MAXNAN, R_MAXNAN, R_MAXNAN, R_MAX, R_MAXNAN};
    dsb_reduce<5>(a, op, C.red);
    primal = dsb_dmax(dsb_dmax(dsb_dmax(a[0], a[1]), a[2]), a[3]);
    dual = a[4];
}

// update_residuals_nr :516-624
__device__ __forceinline__ void dsb_update_nr(const DsbCtx& C)
{
    const int n = C.n, p = C.p, m = C.m, t = C.t;
    const DsbVars &r = C.r, &nr = C.nr;
    double* wx = C.st.x;    // work_x
    double* wz = C.st.z_l;  // work_z
    __syncthreads();
    for (int j = t; j < p; j += DSB_T) nr.y[j] = kb_gemv_t_col(j, n, C.AT, r.x, -1.0);
    for (int i = t; i < n; i += DSB_T) wx[i] = kb_gemv_n_row(i, n, p, C.AT, r.y, 1.0);
    for (int j = t; j < m; j += DSB_T) {
        wz[j] = r.z_u[j] - r.z_l[j];
        const double g = kb_gemv_t_col(j, n, C.GT, r.x, 1.0);
        nr.z_l[j] = g;
        nr.z_u[j] = -g;
    }
    __syncthreads();
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // dual_rel_norm: three parts; primal_rel_norm: two parts and the signed one
    for (int i = t; i < n; i += DSB_T) {
        const double w2 = kb_gemv_n_row(i, n, m, C.GT, wz, 1.0);
        wx[i] = wx[i] + w2;
        const double v = kb_eval_P_row(i, n, C.Pu, -1.0, r.x);
        nr.x[i] = v;
        a[0] = dsb_comb(a[0], fabs(v * C.ci * C.pdi[i]), R_MAXNAN);
    }
    __syncthreads();
    {
        const double* ca = t == 0 ? r.x : t == 1 ? C.c : t == 2 ? C.b : t == 3 ? C.h_l : t == 4 ? C.h_u : t == 5 ? C.x_l : C.x_u;
        const double* cb = t == 0 ? nr.x : t == 1 ? r.x : t == 2 ? r.y : t == 3 ? r.z_l : t == 4 ? r.z_u : t == 5 ? r.z_bl : r.z_bu;
        const int len = t < 2 ? n : t == 2 ? p : t < 5 ? m : t == 5 ? C.nxl : t == 6 ? C.nxu : 0;
        const double s = dsb_dot(ca, cb, len);
        if (t < 7) C.sc[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        pq_info& I = C.S->info;
        const double ci = C.ci;
        double tmp = -C.sc[0];
        I.primal_obj = 0.5 * tmp;
        I.dual_obj = -0.5 * tmp;
        double dg = ci * fabs(tmp);
        tmp = C.sc[1];
        I.primal_obj += tmp;
        dg = dsb_dmax(dg, ci * fabs(tmp));
        tmp = C.sc[2];
        I.dual_obj -= tmp;
        dg = dsb_dmax(dg, ci * fabs(tmp));
        tmp = -C.sc[3];
        I.dual_obj -= tmp;
        dg = dsb_dmax(dg, ci * fabs(tmp));
        tmp = C.sc[4];
        I.dual_obj -= tmp;
        dg = dsb_dmax(dg, ci * fabs(tmp));
        tmp = -C.sc[5];
        I.dual_obj -= tmp;
        dg = dsb_dmax(dg, ci * fabs(tmp));
        tmp = C.sc[6];
        I.dual_obj -= tmp;
        dg = dsb_dmax(dg, ci * fabs(tmp));
        I.duality_gap = fabs(I.primal_obj - I.dual_obj);
        I.primal_obj = ci * I.primal_obj;
        I.dual_obj = ci * I.dual_obj;
        I.duality_gap = ci * I.duality_gap;
        I.duality_gap_rel = I.duality_gap / dsb_dmax(1.0, dg);
    }
    for (int i = t; i < n; i += DSB_T) {
        nr.x[i] = nr.x[i] - C.c[i];
        a[1] = dsb_comb(a[1], fabs(C.c[i] * C.ci * C.pdi[i]), R_MAXNAN);
    }
    for (int i = t; i < C.nxl; i += DSB_T) { const int idx = C.xl_idx[i]; wx[idx] = wx[idx] - C.xbs[idx] * r.z_bl[i]; }
    __syncthreads();
    for (int i = t; i < C.nxu; i += DSB_T) { const int idx = C.xu_idx[i]; wx[idx] = wx[idx] + C.xbs[idx] * r.z_bu[i]; }
    __syncthreads();
    for (int i = t; i < n; i += DSB_T) {
        a[2] = dsb_comb(a[2], fabs(wx[i] * C.ci * C.pdi[i]), R_MAXNAN);
        nr.x[i] = nr.x[i] - wx[i];
    }
    for (int j = t; j < p; j += DSB_T) {
        a[3] = dsb_comb(a[3], fabs(nr.y[j] * 1.0 * C.pdi[n + j]), R_MAXNAN);
        nr.y[j] = nr.y[j] + C.b[j];
        a[4] = dsb_comb(a[4], fabs(C.b[j] * 1.0 * C.pdi[n + j]), R_MAXNAN);
    }
    for (int j = t; j < m; j += DSB_T) {  // :575-598: the maximum is taken with the SIGNED scaled values
        const double dzi = C.pdi[n + p + j];
        if (C.has_l[j] >= 0) {
            a[5] = dsb_comb(a[5], nr.z_l[j] * dzi, R_MAX);
            nr.z_l[j] = nr.z_l[j] + (-C.h_l[j] - r.s_l[j]);
            a[5] = dsb_comb(a[5], C.h_l[j] * dzi, R_MAX);
            a[5] = dsb_comb(a[5], r.s_l[j] * dzi, R_MAX);
        } else nr.z_l[j] = 0.0;
        if (C.has_u[j] >= 0) {
            a[5] = dsb_comb(a[5], nr.z_u[j] * dzi, R_MAX);
            nr.z_u[j] = nr.z_u[j] + (C.h_u[j] - r.s_u[j]);
            a[5] = dsb_comb(a[5], C.h_u[j] * dzi, R_MAX);
            a[5] = dsb_comb(a[5], r.s_u[j] * dzi, R_MAX);
        } else nr.z_u[j] = 0.0;
    }
    for (int i = t; i < C.nxl; i += DSB_T) {
        const int idx = C.xl_idx[i];
        const double v = C.xbs[idx] * r.x[idx], dbi = C.pdbi[idx];
        a[5] = dsb_comb(a[5], v * dbi, R_MAX);
        a[5] = dsb_comb(a[5], C.x_l[i] * dbi, R_MAX);
        a[5] = dsb_comb(a[5], r.s_bl[i] * dbi, R_MAX);
        nr.z_bl[i] = v + (-C.x_l[i] - r.s_bl[i]);
    }
    for (int i = t; i < C.nxu; i += DSB_T) {
        const int idx = C.xu_idx[i];
        const double v = -C.xbs[idx] * r.x[idx], dbi = C.pdbi[idx];
        a[5] = dsb_comb(a[5], v * dbi, R_MAX);
        a[5] = dsb_comb(a[5], C.x_u[i] * dbi, R_MAX);
        a[5] = dsb_comb(a[5], r.s_bu[i] * dbi, R_MAX);
        nr.z_bu[i] = v + (C.x_u[i] - r.s_bu[i]);
    }
    const int op[6] = {R_MAXNAN, R_MAXNAN, R_MAXNAN, R_MAXNAN, R_MAXNAN, R_MAX};
    dsb_reduce<6>(a, op, C.red);
    const double dual_rel_norm = dsb_dmax(dsb_dmax(a[0], a[1]), a[2]);
    const double primal_rel_norm = dsb_dmax(dsb_dmax(a[3], a[4]), a[5]);
    double pr, dr;
    dsb_res_norms(C, nr, pr, dr);
    if (t == 0) {
        pq_info& I = C.S->info;
        I.prev_primal_res = I.primal_res;
        I.prev_dual_res = I.dual_res;
        I.primal_res = pr;
        I.primal_res_rel = pr / dsb_dmax(1.0, primal_rel_norm);
        I.dual_res = dr;
        I.dual_res_rel = dr / dsb_dmax(1.0, dual_rel_norm);
    }
    __syncthreads();
}

// update_residuals_r :627-647
__device__ __forceinline__ void dsb_update_r(const DsbCtx& C)
{
    const int n = C.n, p = C.p, m = C.m, t = C.t;
    const DsbVars &r = C.r, &nr = C.nr, &res = C.res, &px = C.px;
    __syncthreads();
    const double rho = C.S->info.rho, delta = C.S->info.delta;
    double e[2] = {0.0, 0.0};  // primal_prox_inf, dual_prox_inf :496-513
    for (int i = t; i < n; i += DSB_T) {
        res.x[i] = nr.x[i] - rho * (r.x[i] - px.x[i]);
        e[1] = dsb_comb(e[1], fabs((r.x[i] - px.x[i]) * C.pd[i]), R_MAX);
    }
    for (int j = t; j < p; j += DSB_T) {
        res.y[j] = nr.y[j] - delta * (px.y[j] - r.y[j]);
        e[0] = dsb_comb(e[0], fabs((px.y[j] - r.y[j]) * C.ci * C.pd[n + j]), R_MAX);
    }
    for (int j = t; j < m; j += DSB_T) {
        res.z_l[j] = nr.z_l[j] - delta * (px.z_l[j] - r.z_l[j]);
        res.z_u[j] = nr.z_u[j] - delta * (px.z_u[j] - r.z_u[j]);
        e[0] = dsb_comb(e[0], fabs((px.z_l[j] - r.z_l[j]) * C.ci * C.pd[n + p + j]), R_MAX);
        e[0] = dsb_comb(e[0], fabs((px.z_u[j] - r.z_u[j]) * C.ci * C.pd[n + p + j]), R_MAX);
    }
    for (int i = t; i < C.nxl; i += DSB_T) {
        res.z_bl[i] = nr.z_bl[i] - delta * (px.z_bl[i] - r.z_bl[i]);
        e[0] = dsb_comb(e[0], (px.z_bl[i] - r.z_bl[i]) * C.ci * C.pdb[C.xl_idx[i]], R_MAX);
    }
    for (int i = t; i < C.nxu; i += DSB_T) {
        res.z_bu[i] = nr.z_bu[i] - delta * (px.z_bu[i] - r.z_bu[i]);
        e[0] = dsb_comb(e[0], (px.z_bu[i] - r.z_bu[i]) * C.ci * C.pdb[C.xu_idx[i]], R_MAX);
    }
    const int op[2] = {R_MAX, R_MAX};
    dsb_reduce<2>(e, op, C.red);
    double pr, dr;
    dsb_res_norms(C, res, pr, dr);
    if (t == 0) {
        pq_info& I = C.S->info;
        const double primal_rel_scaling = I.primal_res_rel > 0 ? I.primal_res / I.primal_res_rel : 1.0;
        const double dual_rel_scaling = I.dual_res_rel > 0 ? I.dual_res / I.dual_res_rel : 1.0;
        I.primal_res_reg = pr;
        I.primal_res_reg_rel = pr / primal_rel_scaling;
        I.dual_res_reg = dr;
        I.dual_res_reg_rel = dr / dual_rel_scaling;
        I.primal_prox_inf = e[0] * I.delta;
        I.dual_prox_inf = e[1] * I.rho;
    }
    __syncthreads();
}

// calculate_step :451-470
__device__ __forceinline__ void dsb_calc_step(const DsbCtx& C, double& alpha_s, double& alpha_z)
{
    const int t = C.t;
    const DsbVars &r = C.r, &st = C.st;
    double a[2] = {1.0, 1.0};
    __syncthreads();
    for (int i = t; i < C.m; i += DSB_T) {
        if (st.s_l[i] < 0) a[0] = dsb_dmin(a[0], -r.s_l[i] / st.s_l[i]);
        if (st.s_u[i] < 0) a[0] = dsb_dmin(a[0], -r.s_u[i] / st.s_u[i]);
        if (st.z_l[i] < 0) a[1] = dsb_dmin(a[1], -r.z_l[i] / st.z_l[i]);
        if (st.z_u[i] < 0) a[1] = dsb_dmin(a[1], -r.z_u[i] / st.z_u[i]);
    }
    for (int i = t; i < C.nxl; i += DSB_T) {
        if (st.s_bl[i] < 0) a[0] = dsb_dmin(a[0], -r.s_bl[i] / st.s_bl[i]);
        if (st.z_bl[i] < 0) a[1] = dsb_dmin(a[1], -r.z_bl[i] / st.z_bl[i]);
    }
    for (int i = t; i < C.nxu; i += DSB_T) {
        if (st.s_bu[i] < 0) a[0] = dsb_dmin(a[0], -r.s_bu[i] / st.s_bu[i]);
        if (st.z_bu[i] < 0) a[1] = dsb_dmin(a[1], -r.z_bu[i] / st.z_bu[i]);
    }
    const int op[2] = {R_MIN, R_MIN};
    dsb_reduce<2>(a, op, C.red);
    alpha_s = a[0];
    alpha_z = a[1];
}

// lane 0: the instance asks for a factorisation / a solve
__device__ __forceinline__ void dsb_want_factor(DsbState* S) { S->info.n_factor++; }
__device__ __forceinline__ void dsb_want_solve(DsbState* S) { S->info.n_solve++; }

// the retry ladder :693-699, :828-838 after a failed factorisation (lane 0); returns the next request
__device__ __forceinline__ int dsb_ladder(DsbState* S, const pq_settings& set, bool in_loop)
{
    pq_info& I = S->info;
    if (!S->enable_ref) S->enable_ref = 1;
    else if (I.factor_retires < set.max_factor_retires) {
        I.delta *= 100;
        I.rho *= 100;
        I.factor_retires++;
        I.reg_limit = dsb_dmin(10 * I.reg_limit, set.eps_abs);
        if (in_loop) S->reg_changed = 1;
    } else {
        I.status = PQ_NUMERICS;
        S->stage = ST_DONE;
        return WANT_DONE;
    }
    dsb_want_factor(S);
    return WANT_FACTOR;
}

// :763-824: from the loop's head to the factorisation of the next iteration, or to an exit.  Returns the request (uniform).
__device__ __forceinline__ int dsb_loop_head(const DsbCtx& C, const DsbArgs& A, long long inst)
{
    const pq_settings& set = A.set;
    DsbState* S = C.S;
    const int t = C.t;
    __syncthreads();
    const int iter = S->info.iter;
    __syncthreads();
    if (!(iter < set.max_iter)) {
        if (t == 0) { S->info.status = PQ_MAX_ITER_REACHED; S->stage = ST_DONE; }
        return WANT_DONE;
    }
    if (iter == 0) {
        dsb_update_nr(C);
        if (t == 0) { S->info.prev_primal_res = S->info.primal_res; S->info.prev_dual_res = S->info.dual_res; }
    }
    __syncthreads();
    if (t == 0) {
        pq_info& I = S->info;
        if (A.trace && S->trace_rows < A.trace_max) {
            double* row = A.trace + ((size_t)inst * A.trace_max + S->trace_rows) * 11;
            row[0] = I.iter; row[1] = I.primal_obj; row[2] = I.dual_obj; row[3] = I.duality_gap; row[4] = I.primal_res; row[5] = I.dual_res;
            row[6] = I.rho; row[7] = I.delta; row[8] = I.mu; row[9] = I.primal_step; row[10] = I.dual_step;
            S->trace_rows++;
        }
        if ((I.primal_res < set.eps_abs || I.primal_res_rel < set.eps_rel) && (I.dual_res < set.eps_abs || I.dual_res_rel < set.eps_rel) &&
            (!set.check_duality_gap || I.duality_gap < set.eps_duality_gap_abs || I.duality_gap_rel < set.eps_duality_gap_rel)) {
            I.status = PQ_SOLVED;
            S->stage = ST_DONE;
        }
    }
    __syncthreads();
    if (S->stage == ST_DONE) return WANT_DONE;
    dsb_update_r(C);
    if (t == 0) {
        pq_info& I = S->info;
        const int thr_d = set.reg_finetune_dual_update_threshold < 5 ? set.reg_finetune_dual_update_threshold : 5;
        const int thr_p = set.reg_finetune_primal_update_threshold < 5 ? set.reg_finetune_primal_update_threshold : 5;
        if (I.no_dual_update > thr_d && I.primal_prox_inf > set.infeasibility_threshold && (I.primal_res_reg < set.eps_abs || I.primal_res_reg_rel < set.eps_rel)) {
            I.status = PQ_PRIMAL_INFEASIBLE;
            S->stage = ST_DONE;
        } else if (I.no_primal_update > thr_p && I.dual_prox_inf > set.infeasibility_threshold && (I.dual_res_reg < set.eps_abs || I.dual_res_reg_rel < set.eps_rel)) {
            I.status = PQ_DUAL_INFEASIBLE;
            S->stage = ST_DONE;
        }
    }
    __syncthreads();
    if (S->stage == ST_DONE) return WANT_DONE;
    // :805-813 the boundary shift
    const double epsilon = 2.220446049250313e-16;  // DBL_EPSILON
    const DsbVars& r = C.r;
    double sh[3] = {0.0, DSB_INF, DSB_INF};  // shifted (as a maximum), min z_bl, min z_bu
    for (int j = t; j < C.m; j += DSB_T) {
        if (C.has_l[j] >= 0 && r.z_l[j] < epsilon) { r.z_l[j] += epsilon; sh[0] = 1.0; }
        if (C.has_u[j] >= 0 && r.z_u[j] < epsilon) { r.z_u[j] += epsilon; sh[0] = 1.0; }
    }
    for (int i = t; i < C.nxl; i += DSB_T) sh[1] = dsb_dmin(sh[1], r.z_bl[i]);
    for (int i = t; i < C.nxu; i += DSB_T) sh[2] = dsb_dmin(sh[2], r.z_bu[i]);
    const int op[3] = {R_MAX, R_MIN, R_MIN};
    dsb_reduce<3>(sh, op, C.red);
    bool shifted = sh[0] != 0.0;
    if (C.nxl > 0 && sh[1] < epsilon) {
        for (int i = t; i < C.nxl; i += DSB_T) r.z_bl[i] += epsilon;
        shifted = true;
    }
    if (C.nxu > 0 && sh[2] < epsilon) {
        for (int i = t; i < C.nxu; i += DSB_T) r.z_bu[i] += epsilon;
        shifted = true;
    }
    double mu = 0.0;
    if (shifted) mu = dsb_mu(C);
    if (t == 0) {
        pq_info& I = S->info;
        I.iter++;
        if (shifted) I.mu = mu;
        // :815-824 the regularisation fine-tuning
        if ((I.no_primal_update > set.reg_finetune_primal_update_threshold && I.rho == I.reg_limit && I.reg_limit != set.reg_finetune_lower_limit) ||
            (I.no_dual_update > set.reg_finetune_dual_update_threshold && I.delta == I.reg_limit && I.reg_limit != set.reg_finetune_lower_limit)) {
            if (I.dual_prox_inf < set.infeasibility_threshold && I.primal_prox_inf < set.infeasibility_threshold) {
                I.reg_limit = set.reg_finetune_lower_limit;
                I.no_primal_update = 0;
                I.no_dual_update = 0;
            }
        }
        S->reg_changed = 0;
        S->stage = ST_FACTOR;
        dsb_want_factor(S);
    }
    return WANT_FACTOR;
}

// SEL = false: workgroup s is instance s -- the code of before lists of instances existed (A.list is not read).  SEL = true: the grid is sized by the list and a
// workgroup learns its instance from it, by one scalar read; nothing else differs.
template <bool PER, bool SEL>
__global__ __launch_bounds__(DSB_T) void k_dsb_advance(const DsbArgs A)
{
    __shared__ DsbState S;
    __shared__ double sc[16];
    __shared__ double red[DSB_RED];
    __shared__ int s_flag[2];
    const long long inst = SEL ? (long long)A.list[blockIdx.x] : (long long)blockIdx.x;
    const int t = threadIdx.x, n = A.n, p = A.p, m = A.m;
    int* counters = A.counters + 4 * A.slot;
    if (blockIdx.x == 0 && t < 4) A.counters[4 * (A.slot ^ 1) + t] = 0;  // (nobody else touches the other slot during this launch; instance 0 need not be listed)
    {
        const int* src = reinterpret_cast<const int*>(A.state + inst);
        int* dst = reinterpret_cast<int*>(&S);
        for (int i = t; i < (int)(sizeof(DsbState) / sizeof(int)); i += DSB_T) dst[i] = src[i];
    }
    __syncthreads();
    const int stage = S.stage;
    if (stage == ST_DONE) {  // (uniform) an instance that is done is never touched again
        if (t == 0) atomicAdd(counters + WANT_DONE, 1);
        return;
    }
    const size_t on = (size_t)inst * n, op = (size_t)inst * p, om = (size_t)inst * m;
    const pq_settings& set = A.set;
    const KbBounds R = kb_bound_row<PER>(A.bd, inst);
    DsbCtx C;
    C.n = n; C.p = p; C.m = m; C.nxl = R.nxl; C.nxu = R.nxu; C.t = t;
    C.cnt = (double)(R.nhl + R.nhu + R.nxl + R.nxu);
    C.ci = A.pc_inv[inst];
    C.Pu = A.Pu + inst * (size_t)n * n; C.AT = A.AT + inst * (size_t)n * p; C.GT = A.GT + inst * (size_t)n * m;
    C.c = A.c + on; C.b = A.b + op; C.h_l = A.h_l + om; C.h_u = A.h_u + om; C.x_l = A.x_l + on; C.x_u = A.x_u + on; C.xbs = A.xbs + on;
    C.pd = A.pd + (size_t)inst * (n + p + m); C.pdi = A.pdi + (size_t)inst * (n + p + m); C.pdb = A.pdb + on; C.pdbi = A.pdbi + on;
    C.has_l = R.has_l; C.has_u = R.has_u; C.xl_idx = R.xl_idx; C.xu_idx = R.xu_idx;
    C.r = dsb_at(A.r, on, op, om); C.nr = dsb_at(A.nr, on, op, om); C.res = dsb_at(A.res, on, op, om); C.st = dsb_at(A.st, on, op, om); C.px = dsb_at(A.px, on, op, om);
    C.S = &S; C.sc = sc; C.red = red;
    const DsbVars &r = C.r, &res = C.res, &st = C.st, &px = C.px;
    const bool ineq = m + R.nxl + R.nxu > 0;
    int want = WANT_DONE;
    bool to_loop = false;
    __syncthreads();

    if (stage == ST_INIT) {  // :675-690
        if (t == 0) {
            pq_info& I = S.info;
            I.kkt_factor_time = 0; I.kkt_solve_time = 0;
            I.n_factor = I.n_solve = 0; I.n_backend_solve = 0;
            I.status = PQ_UNSOLVED;
            I.iter = 0;
            I.reg_limit = set.reg_lower_limit;
            I.factor_retires = 0; I.no_primal_update = 0; I.no_dual_update = 0;
            I.mu = 0; I.primal_step = 0; I.dual_step = 0;
            I.rho = set.rho_init; I.delta = set.delta_init;
            S.enable_ref = set.iterative_refinement_always_enabled;
            S.trace_rows = 0;
            S.reg_changed = 0;
            S.stage = ST_FACTOR0;
            dsb_want_factor(&S);
        }
        for (int j = t; j < m; j += DSB_T) {
            const double l = R.has_l[j] >= 0 ? 1.0 : 0.0, u = R.has_u[j] >= 0 ? 1.0 : 0.0;
            r.s_l[j] = l; r.z_l[j] = l; r.s_u[j] = u; r.z_u[j] = u;
        }
        for (int i = t; i < R.nxl; i += DSB_T) { r.s_bl[i] = 1.0; r.z_bl[i] = 1.0; }
        for (int i = t; i < R.nxu; i += DSB_T) { r.s_bu[i] = 1.0; r.z_bu[i] = 1.0; }
        want = WANT_FACTOR;
    } else if (stage == ST_FACTOR0 || stage == ST_FACTOR) {
        const bool ok = A.fstatus[inst] == 0;
        if (!ok) {
            if (t == 0) s_flag[0] = dsb_ladder(&S, set, stage == ST_FACTOR);
            __syncthreads();
            want = s_flag[0];
        } else if (stage == ST_FACTOR0) {  // :700-712
            if (t == 0) { S.info.factor_retires = 0; S.stage = ST_SOLVE0; dsb_want_solve(&S); }
            for (int i = t; i < n; i += DSB_T) {
                res.x[i] = -C.c[i];
                res.z_bl[i] = -C.x_l[i]; res.z_bu[i] = C.x_u[i];  // (full length: the entries past the lists are never read)
                res.s_bl[i] = 0.0; res.s_bu[i] = 0.0;
            }
            for (int j = t; j < p; j += DSB_T) res.y[j] = C.b[j];
            for (int j = t; j < m; j += DSB_T) { res.z_l[j] = -C.h_l[j]; res.z_u[j] = C.h_u[j]; res.s_l[j] = 0.0; res.s_u[j] = 0.0; }
            want = WANT_SOLVE;
        } else {  // :839-851, :926
            const bool changed = S.reg_changed != 0;
            __syncthreads();
            if (t == 0) S.info.factor_retires = 0;
            if (changed) dsb_update_r(C);
            if (ineq) {
                for (int j = t; j < m; j += DSB_T) { res.s_l[j] = -r.s_l[j] * r.z_l[j]; res.s_u[j] = -r.s_u[j] * r.z_u[j]; }
                for (int i = t; i < R.nxl; i += DSB_T) res.s_bl[i] = -r.s_bl[i] * r.z_bl[i];
                for (int i = t; i < R.nxu; i += DSB_T) res.s_bu[i] = -r.s_bu[i] * r.z_bu[i];
            }
            if (t == 0) { S.stage = ineq ? ST_PRED : ST_NOINEQ; dsb_want_solve(&S); }
            want = WANT_SOLVE;
        }
    } else {
        // a solve has come back; the reference ignores its success (kkt_solve :656-661): a failed one left `step` as it was
        if (t == 0) S.info.n_backend_solve += A.sinfo[2 * (size_t)A.batch + inst];
        if (stage == ST_SOLVE0) {  // :712-761
            if (A.sinfo[inst] != 0) {  // the reference's first solve writes into result: a copy of bits
                for (int i = t; i < n; i += DSB_T) r.x[i] = st.x[i];
                for (int j = t; j < p; j += DSB_T) r.y[j] = st.y[j];
                for (int j = t; j < m; j += DSB_T) { r.z_l[j] = st.z_l[j]; r.z_u[j] = st.z_u[j]; r.s_l[j] = st.s_l[j]; r.s_u[j] = st.s_u[j]; }
                for (int i = t; i < R.nxl; i += DSB_T) { r.z_bl[i] = st.z_bl[i]; r.s_bl[i] = st.s_bl[i]; }
                for (int i = t; i < R.nxu; i += DSB_T) { r.z_bu[i] = st.z_bu[i]; r.s_bu[i] = st.s_bu[i]; }
            }
            __syncthreads();
            if (ineq) {
                double mn[8];  // min_coeff of s_l, s_u, s_bl, s_bu, z_l, z_u, z_bl, z_bu
                for (int k = 0; k < 8; ++k) mn[k] = DSB_INF * DSB_INF;
                for (int j = t; j < m; j += DSB_T) {
                    mn[0] = dsb_dmin(mn[0], r.s_l[j]); mn[1] = dsb_dmin(mn[1], r.s_u[j]);
                    mn[4] = dsb_dmin(mn[4], r.z_l[j]); mn[5] = dsb_dmin(mn[5], r.z_u[j]);
                }
                for (int i = t; i < R.nxl; i += DSB_T) { mn[2] = dsb_dmin(mn[2], r.s_bl[i]); mn[6] = dsb_dmin(mn[6], r.z_bl[i]); }
                for (int i = t; i < R.nxu; i += DSB_T) { mn[3] = dsb_dmin(mn[3], r.s_bu[i]); mn[7] = dsb_dmin(mn[7], r.z_bu[i]); }
                const int opm[8] = {R_MIN, R_MIN, R_MIN, R_MIN, R_MIN, R_MIN, R_MIN, R_MIN};
                dsb_reduce<8>(mn, opm, red);
                double delta_s = 0.0, delta_z = 0.0;
                if (m > 0) { delta_s = dsb_dmax(delta_s, -mn[0]); delta_s = dsb_dmax(delta_s, -mn[1]); }
                if (R.nxl > 0) delta_s = dsb_dmax(delta_s, -mn[2]);
                if (R.nxu > 0) delta_s = dsb_dmax(delta_s, -mn[3]);
                if (m > 0) { delta_z = dsb_dmax(delta_z, -mn[4]); delta_z = dsb_dmax(delta_z, -mn[5]); }
                if (R.nxl > 0) delta_z = dsb_dmax(delta_z, -mn[6]);
                if (R.nxu > 0) delta_z = dsb_dmax(delta_z, -mn[7]);
                for (int j = t; j < m; j += DSB_T) {
                    if (R.has_l[j] >= 0) { r.s_l[j] += delta_s; r.z_l[j] += delta_z; }
                    if (R.has_u[j] >= 0) { r.s_u[j] += delta_s; r.z_u[j] += delta_z; }
                }
                for (int i = t; i < R.nxl; i += DSB_T) { r.s_bl[i] += delta_s; r.z_bl[i] += delta_z; }
                for (int i = t; i < R.nxu; i += DSB_T) { r.s_bu[i] += delta_s; r.z_bu[i] += delta_z; }
                double mu = dsb_dmax(dsb_mu(C), 1e-10);
                for (int j = t; j < m; j += DSB_T) {
                    if (R.has_l[j] >= 0) {
                        const double c = r.z_l[j] - delta_z;
                        r.z_l[j] = (c + sqrt(c * c + 4 * mu)) / 2;
                        r.s_l[j] = r.z_l[j] - c;
                    }
                    if (R.has_u[j] >= 0) {
                        const double c = r.z_u[j] - delta_z;
                        r.z_u[j] = (c + sqrt(c * c + 4 * mu)) / 2;
                        r.s_u[j] = r.z_u[j] - c;
                    }
                }
                for (int i = t; i < R.nxl; i += DSB_T) {
                    const double c = r.z_bl[i] - delta_z;
                    r.z_bl[i] = (c + sqrt(c * c + 4 * mu)) / 2;
                    r.s_bl[i] = r.z_bl[i] - c;
                }
                for (int i = t; i < R.nxu; i += DSB_T) {
                    const double c = r.z_bu[i] - delta_z;
                    r.z_bu[i] = (c + sqrt(c * c + 4 * mu)) / 2;
                    r.s_bu[i] = r.z_bu[i] - c;
                }
                mu = dsb_mu(C);
                if (t == 0) S.info.mu = mu;
            }
            for (int i = t; i < n; i += DSB_T) px.x[i] = r.x[i];
            for (int j = t; j < p; j += DSB_T) px.y[j] = r.y[j];
            for (int j = t; j < m; j += DSB_T) { px.z_l[j] = r.z_l[j]; px.z_u[j] = r.z_u[j]; }
            for (int i = t; i < R.nxl; i += DSB_T) px.z_bl[i] = r.z_bl[i];
            for (int i = t; i < R.nxu; i += DSB_T) px.z_bu[i] = r.z_bu[i];
            to_loop = true;
        } else if (stage == ST_PRED) {  // :854-879
            double alpha_s, alpha_z;
            dsb_calc_step(C, alpha_s, alpha_z);
            alpha_s *= set.tau;
            alpha_z *= set.tau;
            {
                const double* s0 = t == 0 ? r.s_l : t == 1 ? r.s_u : t == 2 ? r.s_bl : r.s_bu;
                const double* s1 = t == 0 ? st.s_l : t == 1 ? st.s_u : t == 2 ? st.s_bl : st.s_bu;
                const double* z0 = t == 0 ? r.z_l : t == 1 ? r.z_u : t == 2 ? r.z_bl : r.z_bu;
                const double* z1 = t == 0 ? st.z_l : t == 1 ? st.z_u : t == 2 ? st.z_bl : st.z_bu;
                const int len = t < 2 ? m : t == 2 ? R.nxl : t == 3 ? R.nxu : 0;
                double acc = 0.0;
                for (int i = 0; i < len; ++i) acc += (s0[i] + alpha_s * s1[i]) * (z0[i] + alpha_z * z1[i]);
                if (t < 4) sc[t] = acc;
            }
            __syncthreads();
            const double mu0 = S.info.mu;
            double sigma = sc[0];
            sigma += sc[1];
            sigma += sc[2];
            sigma += sc[3];
            sigma /= (mu0 * C.cnt);
            sigma = dsb_dmax(0.0, dsb_dmin(1.0, sigma));
            sigma = sigma * sigma * sigma;
            const double sm = sigma * mu0;
            __syncthreads();
            if (t == 0) { S.info.sigma = sigma; S.stage = ST_CORR; dsb_want_solve(&S); }
            for (int j = t; j < m; j += DSB_T) { res.s_l[j] += -st.s_l[j] * st.z_l[j] + sm; res.s_u[j] += -st.s_u[j] * st.z_u[j] + sm; }
            for (int i = t; i < R.nxl; i += DSB_T) res.s_bl[i] += -st.s_bl[i] * st.z_bl[i] + sm;
            for (int i = t; i < R.nxu; i += DSB_T) res.s_bu[i] += -st.s_bu[i] * st.z_bu[i] + sm;
            want = WANT_SOLVE;
        } else {  // ST_CORR :882-924, ST_NOINEQ :929-948
            double ps = 1.0, ds = 1.0;
            if (stage == ST_CORR) {
                double alpha_s, alpha_z;
                dsb_calc_step(C, alpha_s, alpha_z);
                ps = alpha_s * set.tau;
                ds = alpha_z * set.tau;
            }
            __syncthreads();
            if (t == 0) { S.info.primal_step = ps; S.info.dual_step = ds; }
            for (int i = t; i < n; i += DSB_T) r.x[i] += ps * st.x[i];
            for (int j = t; j < p; j += DSB_T) r.y[j] += ds * st.y[j];
            double mu_rate = 0.0;
            if (stage == ST_CORR) {
                for (int j = t; j < m; j += DSB_T) { r.z_l[j] += ds * st.z_l[j]; r.z_u[j] += ds * st.z_u[j]; r.s_l[j] += ps * st.s_l[j]; r.s_u[j] += ps * st.s_u[j]; }
                for (int i = t; i < R.nxl; i += DSB_T) { r.z_bl[i] += ds * st.z_bl[i]; r.s_bl[i] += ps * st.s_bl[i]; }
                for (int i = t; i < R.nxu; i += DSB_T) { r.z_bu[i] += ds * st.z_bu[i]; r.s_bu[i] += ps * st.s_bu[i]; }
                __syncthreads();
                const double mu_prev = S.info.mu;
                const double mu = dsb_mu(C);
                if (t == 0) S.info.mu = mu;
                mu_rate = dsb_dmax(0.0, (mu_prev - mu) / mu_prev);
            }
            dsb_update_nr(C);
            if (t == 0) {
                pq_info& I = S.info;
                const bool c = stage == ST_CORR;
                int cx = 0, cy = 0;
                if (I.dual_res < 0.95 * I.prev_dual_res || (I.dual_res < set.eps_abs || I.dual_res_rel < set.eps_rel) ||
                    (c && I.rho == set.reg_finetune_lower_limit && I.dual_prox_inf < set.infeasibility_threshold)) {
                    cx = 1;
                    I.rho = dsb_dmax(I.reg_limit, c ? (1.0 - mu_rate) * I.rho : 0.1 * I.rho);
                } else {
                    I.no_primal_update++;
                    if (I.iter < 5 || I.dual_prox_inf < set.infeasibility_threshold) I.rho = dsb_dmax(I.reg_limit, c ? (1.0 - 0.666 * mu_rate) * I.rho : 0.5 * I.rho);
                }
                if (I.primal_res < 0.95 * I.prev_primal_res || (I.primal_res < set.eps_abs || I.primal_res_rel < set.eps_rel) ||
                    (c && I.delta == set.reg_finetune_lower_limit && I.primal_prox_inf < set.infeasibility_threshold)) {
                    cy = 1;
                    I.delta = dsb_dmax(I.reg_limit, c ? (1.0 - mu_rate) * I.delta : 0.1 * I.delta);
                } else {
                    I.no_dual_update++;
                    if (I.iter < 5 || I.primal_prox_inf < set.infeasibility_threshold) I.delta = dsb_dmax(I.reg_limit, c ? (1.0 - 0.666 * mu_rate) * I.delta : 0.5 * I.delta);
                }
                s_flag[0] = cx;
                s_flag[1] = cy;
            }
            __syncthreads();
            if (s_flag[0])
                for (int i = t; i < n; i += DSB_T) px.x[i] = r.x[i];
            if (s_flag[1]) {
                for (int j = t; j < p; j += DSB_T) px.y[j] = r.y[j];
                if (stage == ST_CORR) {
                    for (int j = t; j < m; j += DSB_T) { px.z_l[j] = r.z_l[j]; px.z_u[j] = r.z_u[j]; }
                    for (int i = t; i < R.nxl; i += DSB_T) px.z_bl[i] = r.z_bl[i];
                    for (int i = t; i < R.nxu; i += DSB_T) px.z_bu[i] = r.z_bu[i];
                }
            }
            to_loop = true;
        }
    }
    if (to_loop) want = dsb_loop_head(C, A, inst);
    __syncthreads();
    if (t == 0) {
        if (want == WANT_FACTOR) { A.rho[inst] = S.info.rho; A.delta[inst] = S.info.delta; A.flags[inst] = S.enable_ref; }
        A.act_f[inst] = want == WANT_FACTOR;
        A.act_s[inst] = want == WANT_SOLVE;
        atomicAdd(counters + want, 1);
    }
    {
        int* dst = reinterpret_cast<int*>(A.state + inst);
        const int* src = reinterpret_cast<const int*>(&S);
        for (int i = t; i < (int)(sizeof(DsbState) / sizeof(int)); i += DSB_T) dst[i] = src[i];
    }
}

// ---- unscale_results and restore_dual :956-986, into the result arrays (full length, boxes expanded)
struct DsbFinishArgs {
    int n, p, m;
    KbBounds bd;
    const double *pd, *pdb, *pdi, *pdbi, *pc_inv;
    pq_vars r, out;
    const int* list;  // null: workgroup s is instance s; else one workgroup per entry, workgroup s is instance list[s]
};
template <bool PER>
__global__ __launch_bounds__(DSB_T) void k_dsb_finish(const DsbFinishArgs A)
{
    const long long inst = A.list ? (long long)A.list[blockIdx.x] : (long long)blockIdx.x;
    const int t = threadIdx.x, n = A.n, p = A.p, m = A.m;
    const size_t on = (size_t)inst * n, op = (size_t)inst * p, om = (size_t)inst * m;
    const DsbVars r = dsb_at(A.r, on, op, om), o = dsb_at(A.out, on, op, om);
    const KbBounds R = kb_bound_row<PER>(A.bd, inst);
    const double* pd = A.pd + (size_t)inst * (n + p + m);
    const double* pdi = A.pdi + (size_t)inst * (n + p + m);
    const double ci = A.pc_inv[inst];
    for (int i = t; i < n; i += DSB_T) {
        o.x[i] = r.x[i] * pd[i];
        o.z_bl[i] = 0.0; o.s_bl[i] = DSB_INF; o.z_bu[i] = 0.0; o.s_bu[i] = DSB_INF;
    }
    for (int j = t; j < p; j += DSB_T) o.y[j] = r.y[j] * ci * pd[n + j];
    for (int j = t; j < m; j += DSB_T) {
        const double zl = r.z_l[j] * ci * pd[n + p + j], zu = r.z_u[j] * ci * pd[n + p + j];
        o.z_l[j] = zl;
        o.z_u[j] = zu;
        o.s_l[j] = zl == 0 ? DSB_INF : r.s_l[j] * pdi[n + p + j];
        o.s_u[j] = zu == 0 ? DSB_INF : r.s_u[j] * pdi[n + p + j];
    }
    __syncthreads();
    for (int i = t; i < R.nxl; i += DSB_T) {
        const int idx = R.xl_idx[i];
        o.z_bl[idx] = r.z_bl[i] * ci * A.pdb[on + idx];
        o.s_bl[idx] = r.s_bl[i] * A.pdbi[on + idx];
    }
    for (int i = t; i < R.nxu; i += DSB_T) {
        const int idx = R.xu_idx[i];
        o.z_bu[idx] = r.z_bu[i] * ci * A.pdb[on + idx];
        o.s_bu[idx] = r.s_bu[i] * A.pdbi[on + idx];
    }
}

// ---- the data of a setup: upper(P), A' and G' column-major from the caller's stacks
// mode 0: dst = src (a row-major A is the column-major A'); 1: transpose of a column-major rows x n matrix; 2: upper triangle of a column-major P; 3: of a row-major P.
// dead: columns of the result that are zeroed (rows of G without a finite bound); row `row` of the call reads dead[row * dead_stride + column]: stride 0 at setup, where
// the batch shares the mask, `cols` at an update, where an instance may give both bounds of a row infinite and another not.
// list: null = row `row` of src is instance `row`; else total counts the rows of the list and row `row` of src goes to instance list[row].  ONE indexing for the
// mask in every kernel of an update: `dead` goes by the ROW OF THE CALL, like src (without a list that is the instance); dst alone goes by instance.
__global__ void k_dsb_ingest(const double* __restrict__ src, double* __restrict__ dst, int n, int cols, long long total, int mode, const int* __restrict__ dead,
                             int dead_stride, const int* __restrict__ list)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long long per = (long long)n * cols, row = e / per;
    const int q = (int)(e % per), i = q % n, j = q / n;
    const double* s = src + row * per;
    double v;
    if (mode == 0) v = s[q];
    else if (mode == 1) v = s[j + (size_t)i * cols];
    else if (mode == 2) v = i <= j ? s[q] : 0.0;
    else v = i <= j ? s[j + (size_t)i * n] : 0.0;
    if (dead && dead[row * dead_stride + j]) v = 0.0;
    dst[(list ? (long long)list[row] : row) * per + q] = v;
}

// ---- RuizEquilibration::unscale_data, dense (orc_solver.c:243-256), one workgroup per instance, in place: the first step of an update
// dead: null, or [rows of the call][m]: the columns of G' that disable_inf_constraints zeroes in this update (a row whose two bounds are both given infinite); it
// goes by the row of the call (blockIdx.x), as in k_dsb_ingest.  list: as DsbFinishArgs::list
struct DsbUnscaleArgs {
    int n, p, m;
    KbBounds bd;  // the tables as they stood BEFORE this update: the stored box vectors are packed to them
    double *Pu, *AT, *GT, *c, *b, *h_l, *h_u, *x_l, *x_u, *xbs;
    const double *pdi, *pdbi, *pc_inv;
    const int* dead;
    const int* list;
};
template <bool PER>
__global__ __launch_bounds__(DSB_RUIZ_T) void k_dsb_unscale(const DsbUnscaleArgs A)
{
    const long long inst = A.list ? (long long)A.list[blockIdx.x] : (long long)blockIdx.x;
    const int t = threadIdx.x, T = DSB_RUIZ_T, n = A.n, p = A.p, m = A.m, N = n + p + m;
    double* P = A.Pu + inst * (size_t)n * n;
    double* AT = A.AT + inst * (size_t)n * p;
    double* GT = A.GT + inst * (size_t)n * m;
    double *c = A.c + inst * (size_t)n, *b = A.b + inst * (size_t)p, *h_l = A.h_l + inst * (size_t)m, *h_u = A.h_u + inst * (size_t)m;
    double *x_l = A.x_l + inst * (size_t)n, *x_u = A.x_u + inst * (size_t)n, *xbs = A.xbs + inst * (size_t)n;
    const double *di = A.pdi + inst * (size_t)N, *dib = A.pdbi + inst * (size_t)n;
    const int* dead = A.dead ? A.dead + blockIdx.x * (size_t)m : nullptr;
    const double ci = A.pc_inv[inst];
    const KbBounds R = kb_bound_row<PER>(A.bd, inst);
    for (int e = t; e < n * n; e += T) {  // scale_P_scalar, then scale_P: the column pass, the row pass (the lower triangle is zero and stays zero)
        const int i = e % n, j = e / n;
        if (i <= j) P[e] = ((P[e] * ci) * di[j]) * di[i];
    }
    for (int i = t; i < n; i += T) {
        c[i] = c[i] * (ci * di[i]);
        xbs[i] = xbs[i] * (dib[i] * di[i]);
    }
    for (int e = t; e < n * p; e += T) AT[e] = (di[e % n] * AT[e]) * di[n + e / n];
    for (size_t e = t; e < (size_t)n * m; e += T) GT[e] = dead && dead[e / n] ? 0.0 : (di[e % n] * GT[e]) * di[n + p + e / n];
    for (int i = t; i < p; i += T) b[i] = b[i] * di[n + i];
    for (int i = t; i < m; i += T) {  // (a row dropped in this update: -1 / 1 on both sides, also on the side the caller did not give)
        const bool dd = dead && dead[i];
        h_l[i] = dd ? -1.0 : h_l[i] * di[n + p + i];
        h_u[i] = dd ? 1.0 : h_u[i] * di[n + p + i];
    }
    for (int i = t; i < R.nxl; i += T) x_l[i] = x_l[i] * dib[R.xl_idx[i]];
    for (int i = t; i < R.nxu; i += T) x_u[i] = x_u[i] * dib[R.xu_idx[i]];
}

// ---- RuizEquilibration::scale_data, dense (orc_solver.c:136-240), one workgroup per instance, in place.  reuse = 0: the equilibration from delta = 1 (a setup; an
// update that gave a matrix with preconditioner_reuse_on_update off: xbs is read as it stands).  reuse = 1: the stored scalings are applied (:229-235) and they, their
// inverses and c stay untouched.  Both end in the one tail :236-239.
struct DsbRuizArgs {
    int n, p, m, max_iter, scale_cost, reuse;
    KbBounds bd;
    double epsilon;
    double *Pu, *AT, *GT, *c, *b, *h_l, *h_u, *x_l, *x_u, *xbs;
    double *pd, *pdb, *pdi, *pdbi, *pc, *pc_inv;
    const int* list;  // as DsbArgs::list
};
__device__ __forceinline__ double dsb_limit_scaling(double d) { return d < 1e-4 ? 1.0 : (d > 1e4 ? 1e4 : d); }

template <bool PER, bool SEL>  // (SEL: as at k_dsb_advance)
__global__ __launch_bounds__(DSB_RUIZ_T) void k_dsb_ruiz(const DsbRuizArgs A)
{
    __shared__ double red[DSB_RED];
    __shared__ double colmax[PQ_KKT_BATCH_DENSE_MAX_N];
    __shared__ double s_gamma;
    const long long inst = SEL ? (long long)A.list[blockIdx.x] : (long long)blockIdx.x;
    const int t = threadIdx.x, T = DSB_RUIZ_T, n = A.n, p = A.p, m = A.m, N = n + p + m;
    double* P = A.Pu + inst * (size_t)n * n;
    double* AT = A.AT + inst * (size_t)n * p;
    double* GT = A.GT + inst * (size_t)n * m;
    double *c = A.c + inst * (size_t)n, *b = A.b + inst * (size_t)p, *h_l = A.h_l + inst * (size_t)m, *h_u = A.h_u + inst * (size_t)m;
    double *x_l = A.x_l + inst * (size_t)n, *x_u = A.x_u + inst * (size_t)n, *xbs = A.xbs + inst * (size_t)n;
    double *delta = A.pd + inst * (size_t)N, *di = A.pdi + inst * (size_t)N, *delta_b = A.pdb + inst * (size_t)n, *dib = A.pdbi + inst * (size_t)n;
    const KbBounds R = kb_bound_row<PER>(A.bd, inst);
    double rc = 1.0;
    if (A.reuse) {
        rc = A.pc[inst];
        for (int e = t; e < n * n; e += T) {  // scale_P_scalar, then scale_P
            const int i = e % n, j = e / n;
            if (i <= j) P[e] = ((P[e] * rc) * delta[j]) * delta[i];
        }
        for (int i = t; i < n; i += T) {
            c[i] = c[i] * (rc * delta[i]);
            xbs[i] = xbs[i] * (delta_b[i] * delta[i]);
        }
        for (int e = t; e < n * p; e += T) AT[e] = (delta[e % n] * AT[e]) * delta[n + e / n];
        for (size_t e = t; e < (size_t)n * m; e += T) GT[e] = (delta[e % n] * GT[e]) * delta[n + p + e / n];
    } else {
        for (int i = t; i < N; i += T) { delta[i] = 1.0; di[i] = 0.0; }
        for (int i = t; i < n; i += T) { delta_b[i] = 1.0; dib[i] = 0.0; }
    }
    __syncthreads();
    for (int it = 0; it < (A.reuse ? 0 : A.max_iter); ++it) {
        double dev[1] = {0.0};
        for (int i = t; i < N; i += T) dev[0] = dsb_dmax(dev[0], fabs(1.0 - di[i]));
        for (int i = t; i < n; i += T) dev[0] = dsb_dmax(dev[0], fabs(1.0 - dib[i]));
        const int opd[1] = {R_MAX};
        dsb_reduce<1>(dev, opd, red);
        if (!(dev[0] > A.epsilon)) break;  // (uniform)
        for (int k = t; k < n; k += T) {
            double v = 0.0;
            for (int i = 0; i < k; ++i) v = dsb_dmax(v, fabs(P[i + (size_t)k * n]));
            for (int j = k; j < n; ++j) v = dsb_dmax(v, fabs(P[k + (size_t)j * n]));
            for (int j = 0; j < p; ++j) v = dsb_dmax(v, fabs(AT[k + (size_t)j * n]));
            for (int j = 0; j < m; ++j) v = dsb_dmax(v, fabs(GT[k + (size_t)j * n]));
            v = dsb_dmax(v, xbs[k]);
            di[k] = v;
        }
        for (int k = t; k < p; k += T) {
            double v = 0.0;
            for (int i = 0; i < n; ++i) v = dsb_dmax(v, fabs(AT[i + (size_t)k * n]));
            di[n + k] = v;
        }
        for (int k = t; k < m; k += T) {
            double v = 0.0;
            for (int i = 0; i < n; ++i) v = dsb_dmax(v, fabs(GT[i + (size_t)k * n]));
            di[n + p + k] = v;
        }
        for (int i = t; i < n; i += T) dib[i] = xbs[i];
        __syncthreads();
        for (int i = t; i < N; i += T) di[i] = 1.0 / sqrt(dsb_limit_scaling(di[i]));
        for (int i = t; i < n; i += T) dib[i] = 1.0 / sqrt(dsb_limit_scaling(dib[i]));
        __syncthreads();
        for (int e = t; e < n * n; e += T) {  // scale_P :102-108: the column pass, then the row pass
            const int i = e % n, j = e / n;
            if (i <= j) P[e] = (P[e] * di[j]) * di[i];
        }
        for (int i = t; i < n; i += T) c[i] = c[i] * di[i];
        for (int e = t; e < n * p; e += T) AT[e] = (di[e % n] * AT[e]) * di[n + e / n];
        for (size_t e = t; e < (size_t)n * m; e += T) GT[e] = (di[e % n] * GT[e]) * di[n + p + e / n];
        for (int i = t; i < n; i += T) {
            xbs[i] = xbs[i] * (dib[i] * di[i]);
            delta_b[i] = delta_b[i] * dib[i];
        }
        for (int i = t; i < N; i += T) delta[i] = delta[i] * di[i];
        __syncthreads();
        if (A.scale_cost) {
            double cinf[1] = {0.0};
            for (int k = t; k < n; k += T) {
                double a = 0.0, bb = 0.0;
                for (int i = 0; i < k; ++i) a = dsb_dmax(a, fabs(P[i + (size_t)k * n]));
                for (int j = k; j < n; ++j) bb = dsb_dmax(bb, fabs(P[k + (size_t)j * n]));
                colmax[k] = dsb_dmax(a, bb);
                cinf[0] = dsb_dmax(cinf[0], fabs(c[k]));
            }
            dsb_reduce<1>(cinf, opd, red);
            if (t == 0) {
                double gamma = 0.0;
                for (int k = 0; k < n; ++k) gamma += colmax[k];  // (a sequential sum over k)
                gamma /= (double)n;
                gamma = dsb_limit_scaling(gamma);
                gamma = dsb_dmax(gamma, cinf[0]);
                gamma = dsb_limit_scaling(gamma);
                s_gamma = 1.0 / gamma;
            }
            __syncthreads();
            const double gamma = s_gamma;
            for (int e = t; e < n * n; e += T) P[e] = P[e] * gamma;
            for (int i = t; i < n; i += T) c[i] = c[i] * gamma;
            rc = rc * gamma;
            __syncthreads();
        }
    }
    __syncthreads();
    if (!A.reuse) {
        if (t == 0) { A.pc[inst] = rc; A.pc_inv[inst] = 1.0 / rc; }
        for (int i = t; i < N; i += T) di[i] = 1.0 / delta[i];
        for (int i = t; i < n; i += T) dib[i] = 1.0 / delta_b[i];
    }
    for (int i = t; i < p; i += T) b[i] = b[i] * delta[n + i];
    for (int i = t; i < m; i += T) { h_l[i] = h_l[i] * delta[n + p + i]; h_u[i] = h_u[i] * delta[n + p + i]; }
    for (int i = t; i < R.nxl; i += T) x_l[i] = x_l[i] * delta_b[R.xl_idx[i]];
    for (int i = t; i < R.nxu; i += T) x_u[i] = x_u[i] * delta_b[R.xu_idx[i]];
}

// settings.hpp:84-106 verify_settings
bool dsb_verify_settings(const pq_settings& s)
{
    return s.rho_init > 0 && s.delta_init > 0 && s.eps_abs > 0 && s.eps_rel >= 0 && s.eps_duality_gap_abs > 0 && s.eps_duality_gap_rel >= 0 && s.infeasibility_threshold >= 0 &&
           s.reg_lower_limit > 0 && s.reg_finetune_primal_update_threshold >= 0 && s.reg_finetune_dual_update_threshold >= 0 && s.max_iter > 0 && s.max_factor_retires > 0 &&
           s.preconditioner_iter >= 0 && s.tau > 0 && s.tau <= 1 && s.iterative_refinement_eps_abs > 0 && s.iterative_refinement_eps_rel >= 0 &&
           s.iterative_refinement_max_iter >= 0 && s.iterative_refinement_min_improvement_rate >= 1.0 && s.iterative_refinement_static_regularization_eps > 0 &&
           s.iterative_refinement_static_regularization_rel >= 0;
}

struct KsDeleter {
    void operator()(pq_kktsys_batch* k) const { pq_kktsys_batch_destroy(k); }
};

// the ten vectors of a set of variables, [batch][len] each, in one allocation
struct VarSet {
    DBuf<double> buf;
    pq_vars v;
    void alloc(size_t b, size_t n, size_t p, size_t m, hipStream_t st)
    {
        size_t len[10];
        vars_lens(n, p, m, len);
        buf.alloc(b * (5 * n + p + 4 * m));
        buf.zero(st);
        double** f = &v.x;
        size_t off = 0;
        for (int i = 0; i < 10; ++i) { f[i] = buf.p + off; off += b * len[i]; }
    }
};

// everything a setup creates
struct DsbProblem {
    int batch = 0, n = 0, p = 0, m = 0, trace_max = 0;
    // the finite-bound sets (dense/data.hpp:98-207, dsb_bound_lists): `rows` = 1 set shared by the batch, or one per instance.  Host images, sized by the setup:
    bool per_inst = false;
    int rows = 1;
    std::vector<int> cnt_h;      // [rows][4]: n_h_l, n_h_u, n_x_l, n_x_u
    std::vector<int> lists_h;    // four arrays [rows][m], [rows][m], [rows][n], [rows][n] one after the other: the lists, meaningful in their first cnt entries
    std::vector<int> fin_h;      // the same four arrays as flags: the stored vector is finite at this place (a dropped row: on both sides)
    std::vector<int> tab_h;      // [rows] rows of `tab`
    std::vector<int> try_h;      // 2 m + 2 n + 4: the lists and counts of one instance while they are compared with the shared ones
    std::vector<int> dead_h;     // [batch][m]
    std::vector<int> keep_h;     // per instance only: cnt_h and lists_h as they stood before an update, put back if the update fails on its way
    std::vector<char> relisted_h;  // per instance only, [batch]: the instance's lists were replaced by an update and it has not been factored since (a solve that
                                   // includes it factors it in its first round); while any is set the KKT system stays `stale`
    VarSet sets[6];  // result, res_nr, res, step, prox, the results handed out
    DBuf<double> c, b, h_l, h_u, x_l, x_u, xbs, pd, pdb, pdi, pdbi, pc, pc_inv, rho, delta, trace;
    DBuf<int> tab, cnt_d, flags, act, counters;  // tab: has_l[m], has_u[m], x_l_idx, x_u_idx (KbBounds without pos_*); cnt_d: [batch][4], per instance only
    // what an update needs and only a setup may allocate: the staging of a host-fed matrix, the mask of the rows an update drops ([batch][m]; a setup with shared
    // sets uses the first m), and pinned room for the four bound vectors as fetched and as packed (2 batch (2 m + 2 n) doubles)
    DBuf<double> raw;
    DBuf<int> dead_d;
    HBuf<double> bnd_h;
    DBuf<int> sel;  // the list of a call that acts on a list of instances (pq_solver_batch_*_select): `batch` ints, allocated by the first such call -- a setup and a clone leave it empty
    DBuf<DsbState> state;
    HBuf<DsbState> state_h;
    HBuf<int> counters_h;
    Event ev[8];  // advance, factor, solve, finish: begin / end
    std::unique_ptr<pq_kktsys_batch, KsDeleter> ks;  // last: destroyed first, which drains the one stream everything here runs on
    size_t tab_stride() const { return 2 * (size_t)m + (per_inst ? 2 * (size_t)n : (size_t)cnt_h[2] + (size_t)cnt_h[3]); }
    int* list(int k, size_t row) { return lists_h.data() + (k == 0 ? 0 : k == 1 ? (size_t)rows * m : k == 2 ? 2 * (size_t)rows * m : 2 * (size_t)rows * m + (size_t)rows * n) + row * (k < 2 ? m : n); }
    int* fin(int k, size_t row) { return fin_h.data() + (list(k, row) - lists_h.data()); }
    const int* list(int k, size_t row) const { return const_cast<DsbProblem*>(this)->list(k, row); }
    const int* fin(int k, size_t row) const { return const_cast<DsbProblem*>(this)->fin(k, row); }
    KbBounds bounds() const
    {
        KbBounds b;
        b.has_l = tab.p; b.has_u = b.has_l + m; b.pos_l = b.pos_u = tab.p;  // (never read: the solver's kernels do not ask where a variable stands in a box list)
        b.xl_idx = b.has_u + m; b.xu_idx = b.xl_idx + (per_inst ? n : cnt_h[2]);
        b.nhl = cnt_h[0]; b.nhu = cnt_h[1]; b.nxl = cnt_h[2]; b.nxu = cnt_h[3];  // (used with shared sets only)
        b.cnt = per_inst ? cnt_d.p : nullptr;
        b.stride = per_inst ? (int)tab_stride() : 0;
        return b;
    }
    // has_l, has_u and the two box lists of every row of tab_h from lists_h and cnt_h
    void fill_tab()
    {
        const size_t stride = tab_stride();
        std::fill(tab_h.begin(), tab_h.end(), -1);
        for (int r = 0; r < rows; ++r) {
            const int* c = cnt_h.data() + 4 * (size_t)r;
            int* t = tab_h.data() + r * stride;
            for (int e = 0; e < c[0]; ++e) t[list(0, r)[e]] = e;
            for (int e = 0; e < c[1]; ++e) t[(size_t)m + list(1, r)[e]] = e;
            std::copy(list(2, r), list(2, r) + c[2], t + 2 * (size_t)m);
            std::copy(list(3, r), list(3, r) + c[3], t + 2 * (size_t)m + (per_inst ? n : c[2]));
        }
    }
    // the lists as flags
    void fill_fin()
    {
        std::fill(fin_h.begin(), fin_h.end(), 0);
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < 4; ++k)
                for (int e = 0; e < cnt_h[4 * (size_t)r + k]; ++e) fin(k, r)[list(k, r)[e]] = 1;
    }
};

}  // namespace

}  // namespace pq

using namespace pq;

struct pq_solver_batch {
    int device = 0;
    pq_settings settings;
    int trace_max = 0;
    int bound_sets = PQ_BOUND_SETS_SHARED;  // read by the next setup
    bool solved = false, updated = false;
    double update_wall_ms = 0.0, update_device_ms = 0.0;
    double wall_ms = 0.0, device_ms = 0.0, factor_ms = 0.0, solve_ms = 0.0;
    int rounds = 0, launches = 0;
    double clone_wall_ms = 0.0, clone_device_ms = 0.0;  // of the clone call that made this handle (0: it was created)
    pq_info invalid_info;  // what pq_solver_batch_info answers before a setup
    std::unique_ptr<DsbProblem> pr;
};

namespace {

size_t dsb_field_len(const DsbProblem* q, int field)
{
    size_t len[10];
    vars_lens((size_t)q->n, (size_t)q->p, (size_t)q->m, len);
    return len[field];
}

int dsb_check_refine_cap(const pq_settings& s)
{
    if (s.iterative_refinement_max_iter < 0 || s.iterative_refinement_max_iter > KB_MAX_REFINE_ITER)
        return fail(PQ_ERR_INVALID, "dense solver batch: iterative_refinement_max_iter = %d, [0, %d] wanted (the loop runs inside a kernel)", s.iterative_refinement_max_iter,
                    KB_MAX_REFINE_ITER);
    return PQ_OK;
}

// the instances a call acts on: the whole batch (dev = null: row j of the call is instance j), or the list of a _select call -- host: the caller's, checked;
// dev: its copy in the problem's `sel`
struct DsbRows {
    const int *host, *dev;
    int count;
    int inst(int j) const { return host ? host[j] : j; }
};
// the rows of a _select call: the list goes up into `sel`, which the first such call on a problem allocates
DsbRows dsb_rows_select(DsbProblem* q, hipStream_t st, const int* idx, int count)
{
    if (!q->sel.p) q->sel.alloc((size_t)q->batch);
    PQ_HIP(hipMemcpyAsync(q->sel.p, idx, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, st));
    return DsbRows{idx, q->sel.p, count};
}

void dsb_ingest(hipStream_t st, const double* src, double* dst, int rows, int n, int cols, int mode, const int* dead, int dead_stride, const int* list)
{
    const long long total = (long long)rows * n * cols;
    if (total == 0) return;
    k_dsb_ingest<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(src, dst, n, cols, total, mode, dead, dead_stride, list);
    PQ_HIP(hipGetLastError());
}

// one of the caller's matrix stacks (a row per row of the call) into upper(P), A' or G' at `dst` (device, by instance): a host stack goes through the problem's
// staging first
void dsb_matrix(DsbProblem* q, hipStream_t st, const DsbRows& rw, const double* src, double* dst, int cols, int mode, const int* dead, int dead_stride, int mem)
{
    if (!cols) return;
    const double* from = src;
    if (mem == PQ_MEM_HOST) {
        PQ_HIP(hipMemcpyAsync(q->raw.p, src, sizeof(double) * (size_t)rw.count * q->n * cols, hipMemcpyHostToDevice, st));
        from = q->raw.p;
    }
    dsb_ingest(st, from, dst, rw.count, q->n, cols, mode, dead, dead_stride, rw.dev);
}

// one of the caller's vector stacks, [rows of the call][len], into the [batch][len] array at `dst`: the whole batch by one copy; a list by k_kb_scatter_rows,
// a host stack through the problem's staging first (`raw` holds a matrix stack of the batch, so a vector stack of at most `batch` rows fits)
void dsb_vector(DsbProblem* q, hipStream_t st, const DsbRows& rw, const double* src, double* dst, size_t len, int mem)
{
    const size_t bytes = sizeof(double) * (size_t)rw.count * len;
    if (!bytes) return;
    if (!rw.dev) { copy_in(dst, src, bytes, mem, st); return; }
    const double* from = src;
    if (mem == PQ_MEM_HOST) {
        PQ_HIP(hipMemcpyAsync(q->raw.p, src, bytes, hipMemcpyHostToDevice, st));
        from = q->raw.p;
    }
    kb_scatter_rows(st, dst, from, rw.dev, (size_t)rw.count, sizeof(double) * len);
}

// scale_data of every instance of `rw` on the matrices at Pu, AT, GT (device), with the settings as they stand
void dsb_launch_ruiz(const pq_solver_batch* s, DsbProblem* q, hipStream_t st, const DsbRows& rw, double* Pu, double* AT, double* GT, int reuse)
{
    DsbRuizArgs r;
    r.n = q->n; r.p = q->p; r.m = q->m; r.bd = q->bounds(); r.max_iter = s->settings.preconditioner_iter; r.scale_cost = s->settings.preconditioner_scale_cost;
    r.reuse = reuse; r.list = rw.dev;
    r.epsilon = 1e-3;
    r.Pu = Pu; r.AT = AT; r.GT = GT; r.c = q->c.p; r.b = q->b.p; r.h_l = q->h_l.p; r.h_u = q->h_u.p; r.x_l = q->x_l.p; r.x_u = q->x_u.p; r.xbs = q->xbs.p;
    r.pd = q->pd.p; r.pdb = q->pdb.p; r.pdi = q->pdi.p; r.pdbi = q->pdbi.p; r.pc = q->pc.p; r.pc_inv = q->pc_inv.p;
    if (q->per_inst) {
        if (rw.dev) k_dsb_ruiz<true, true><<<rw.count, DSB_RUIZ_T, 0, st>>>(r);
        else k_dsb_ruiz<true, false><<<rw.count, DSB_RUIZ_T, 0, st>>>(r);
    } else if (rw.dev) k_dsb_ruiz<false, true><<<rw.count, DSB_RUIZ_T, 0, st>>>(r);
    else k_dsb_ruiz<false, false><<<rw.count, DSB_RUIZ_T, 0, st>>>(r);
    PQ_HIP(hipGetLastError());
}

// ---- the host logic of dense/data.hpp:98-207 for ONE instance: set_h_l, set_h_u, disable_inf_constraints, set_x_l, set_x_u.  The one copy: setup and update call it
// in both modes of the bound sets, pq_debug_bound_lists hands it out.
//   h_l, h_u [m], x_l, x_u [n]: what the caller gave, any may be null.
//   fin: null for a setup, where a vector that is not given is infinite everywhere.  For an update the four flag vectors of the data as stored ([m], [m], [n], [n]):
//        1 = in the list (a row dropped earlier is stored as -1 / 1, in both lists), 0 = infinite.  A vector that is not given keeps what is stored.
//        ONE RULE IS NOT THE REFERENCE'S: a stored infinite bound IS infinite here.  The reference stores it as -/+ 1e30, scales it with its row and un-scales it at
//        the next update, and (1e30 d) (1 / d) may round to the neighbour of 1e30; disable_inf_constraints compares that NUMBER, so when h_l or h_u comes alone and
//        is infinite on a row whose other side is stored infinite, the reference drops the row or -- by the rounding of that product -- leaves it in neither
//        list, a row without a bound that turns its solves into NaN.  Here the row is dropped.
//   cnt[4], idx[4] ([m], [m], [n], [n]): the counts and the ascending lists.  dead [m]: the rows disable_inf_constraints drops in this call -- both bounds infinite, a
//        given one or a stored one; the row of G is zeroed and the bounds become -1 / 1, so the row is in both lists.  Without h_l and h_u an update does not look at
//        the rows: nothing is dropped.
//   packed[4] ([m], [m], [n], [n]): the vectors as the reference stores them.  A given h vector (every one in a setup) is written at full length: the value, -1 / 1 on a
//        dropped row, -/+ 1e30 where infinite.  An h vector an update does not give is written on the rows dropped in this call only.  A given box vector (every one in a
//        setup) is written at full length: the finite values in list order, then zeros; one an update does not give is not touched.
// idx, dead, packed and their entries may be null: that output is not wanted.
void dsb_bound_lists(int m, int n, const double* h_l, const double* h_u, const double* x_l, const double* x_u, const int* const* fin, int cnt[4], int* const* idx, int* dead,
                     double* const* packed)
{
    const bool setup = !fin, rows = setup || h_l || h_u;
    cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
    for (int j = 0; j < m; ++j) {
        const bool fl = h_l ? h_l[j] > -DSB_INF : (!setup && fin[0][j] != 0), fu = h_u ? h_u[j] < DSB_INF : (!setup && fin[1][j] != 0);
        const bool dd = rows && !fl && !fu;
        const bool in_l = fl || dd, in_u = fu || dd;
        if (dead) dead[j] = dd;
        if (in_l) { if (idx && idx[0]) idx[0][cnt[0]] = j; ++cnt[0]; }
        if (in_u) { if (idx && idx[1]) idx[1][cnt[1]] = j; ++cnt[1]; }
        if (packed && packed[0] && (setup || h_l || dd)) packed[0][j] = dd ? -1.0 : fl ? h_l[j] : -DSB_INF;
        if (packed && packed[1] && (setup || h_u || dd)) packed[1][j] = dd ? 1.0 : fu ? h_u[j] : DSB_INF;
    }
    for (int k = 2; k < 4; ++k) {
        const double* v = k == 2 ? x_l : x_u;
        double* out = packed ? packed[k] : nullptr;
        for (int j = 0; j < n; ++j) {
            const bool f = v ? (k == 2 ? v[j] > -DSB_INF : v[j] < DSB_INF) : (!setup && fin[k][j] != 0);
            if (!f) continue;
            if (idx && idx[k]) idx[k][cnt[k]] = j;
            if (out && v) out[cnt[k]] = v[j];
            ++cnt[k];
        }
        if (out && (setup || v))
            for (int j = cnt[k]; j < n; ++j) out[j] = 0.0;
    }
}

// ---- the checks of the calls that act on a list of instances, before any device call.  fn: the call's name, which opens every text
int dsb_check_list(const char* fn, const pq_solver_batch* s, const int* idx, int count)
{
    if (!s) return fail(PQ_ERR_INVALID, "%s: null handle", fn);
    if (!idx) return fail(PQ_ERR_INVALID, "%s: idx is null", fn);
    if (count < 1) return fail(PQ_ERR_INVALID, "%s: count = %d, count >= 1 wanted", fn, count);
    return PQ_OK;
}
// the handle is set up, every entry is an instance, and -- unique -- none is listed twice (two workgroups on one instance would race)
int dsb_check_entries(const char* fn, const pq_solver_batch* s, const int* idx, int count, bool unique)
{
    if (!s->pr) return fail(PQ_ERR_INVALID, "%s: the handle is not set up (there is no instance to list)", fn);
    const int batch = s->pr->batch;
    for (int j = 0; j < count; ++j)
        if (idx[j] < 0 || idx[j] >= batch) return fail(PQ_ERR_INVALID, "%s: idx[%d] = %d outside [0, %d)", fn, j, idx[j], batch);
    if (!unique) return PQ_OK;
    std::vector<int> first((size_t)batch, -1);
    for (int j = 0; j < count; ++j) {
        if (first[idx[j]] >= 0) return fail(PQ_ERR_INVALID, "%s: idx[%d] = %d is listed twice (idx[%d] too)", fn, j, idx[j], first[idx[j]]);
        first[idx[j]] = j;
    }
    return PQ_OK;
}

void dsb_reset_state(pq_solver_batch* s)
{
    DsbProblem* q = s->pr.get();
    for (int i = 0; i < q->batch; ++i) {
        DsbState& S = q->state_h.p[i];
        std::memset(&S, 0, sizeof(S));
        S.info.rho = s->settings.rho_init;
        S.info.delta = s->settings.delta_init;
    }
}

// ---- clone: the per-handle scalars as they stand (the settings, the trace rows and the bound-set mode a next setup would read, solved / updated and the stored
// times); no device is touched
pq_solver_batch* dsb_clone_scalars(const pq_solver_batch* s)
{
    std::unique_ptr<pq_solver_batch> c(new pq_solver_batch);
    c->device = s->device; c->settings = s->settings; c->trace_max = s->trace_max; c->bound_sets = s->bound_sets;
    c->solved = s->solved; c->updated = s->updated;
    c->update_wall_ms = s->update_wall_ms; c->update_device_ms = s->update_device_ms;
    c->wall_ms = s->wall_ms; c->device_ms = s->device_ms; c->factor_ms = s->factor_ms; c->solve_ms = s->solve_ms;
    c->rounds = s->rounds; c->launches = s->launches;
    c->invalid_info = s->invalid_info;
    return c.release();
}

// the problem of s, instance idx[j] as instance j, into c (the list has been checked).  The KKT system and its backend are cloned by the same list
// (ksb_clone_rows), which is uploaded once, here.  Gathered on the new system's stream: the ten fields of each of the six VarSets (each field is an array of
// [batch][len] inside the set's one allocation, so one gather per field), the scaled vectors, x_b_scaling, the preconditioner, rho, delta, the state records and the
// trace; with sets per instance the rows of tab (2 m + 2 n ints here) and cnt_d.  Shared sets: the one table is copied.  The host images follow by plain loops
// (lists_h and fin_h are four arrays of `rows` rows each).  Sized as a setup sizes them and not copied: flags, the activity words, the counters, raw, dead_d,
// bnd_h, try_h, keep_h and the events.
void dsb_clone_problem(const pq_solver_batch* s, pq_solver_batch* c, const int* idx, int count)
{
    const DsbProblem* q = s->pr.get();
    PQ_HIP(hipSetDevice(s->device));
    DBuf<int> idx_d((size_t)count);
    PQ_HIP(hipMemcpy(idx_d.p, idx, sizeof(int) * (size_t)count, hipMemcpyHostToDevice));
    const auto w0 = std::chrono::steady_clock::now();
    c->clone_device_ms = 0.0;
    const KbSelect sel{idx, idx_d.p, count, &c->clone_device_ms};
    const int n = q->n, p = q->p, m = q->m;
    const size_t B = (size_t)count, N = (size_t)n + p + m;
    std::unique_ptr<DsbProblem> d(new DsbProblem);
    d->batch = count; d->n = n; d->p = p; d->m = m; d->trace_max = q->trace_max; d->per_inst = q->per_inst;
    const int R = d->rows = q->per_inst ? count : 1;
    d->try_h.assign(q->try_h.size(), 0);
    d->dead_h.resize(B * m);
    kb_gather_host(d->dead_h.data(), q->dead_h.data(), idx, count, (size_t)m);
    if (q->per_inst) {
        d->cnt_h.resize(4 * (size_t)R); d->lists_h.resize((size_t)R * (2 * (size_t)m + 2 * (size_t)n)); d->fin_h.resize(d->lists_h.size());
        d->keep_h.assign(d->cnt_h.size() + d->lists_h.size(), 0);
        d->relisted_h.resize(B);
        kb_gather_host(d->relisted_h.data(), q->relisted_h.data(), idx, count, 1);
        kb_gather_host(d->cnt_h.data(), q->cnt_h.data(), idx, count, 4);
        for (int k = 0; k < 4; ++k) {
            kb_gather_host(d->list(k, 0), q->list(k, 0), idx, count, (size_t)(k < 2 ? m : n));
            kb_gather_host(d->fin(k, 0), q->fin(k, 0), idx, count, (size_t)(k < 2 ? m : n));
        }
        d->tab_h.resize((size_t)R * d->tab_stride());
        kb_gather_host(d->tab_h.data(), q->tab_h.data(), idx, count, d->tab_stride());
    } else {
        d->cnt_h = q->cnt_h; d->lists_h = q->lists_h; d->fin_h = q->fin_h; d->tab_h = q->tab_h;
    }
    d->ks.reset(ksb_clone_rows(q->ks.get(), sel));  // (waits for the source's stream first)
    hipStream_t st = ksb_stream(d->ks.get());
    for (Event& e : d->ev) e = Event(0);
    size_t len[10];
    vars_lens((size_t)n, (size_t)p, (size_t)m, len);
    PQ_HIP(hipEventRecord(d->ev[0], st));
    for (int v = 0; v < 6; ++v) {
        d->sets[v].alloc(B, n, p, m, st);
        for (int f = 0; f < 10; ++f) kb_gather_rows(st, vars_field(d->sets[v].v, f), vars_field(q->sets[v].v, f), sel.dev, B, sizeof(double) * len[f]);
    }
    auto rows = [&](DBuf<double>& dst, const DBuf<double>& src, size_t l) {
        dst.alloc(B * l);
        kb_gather_rows(st, dst.p, src.p, sel.dev, B, sizeof(double) * l);
    };
    rows(d->c, q->c, n); rows(d->b, q->b, p); rows(d->h_l, q->h_l, m); rows(d->h_u, q->h_u, m); rows(d->x_l, q->x_l, n); rows(d->x_u, q->x_u, n); rows(d->xbs, q->xbs, n);
    rows(d->pd, q->pd, N); rows(d->pdi, q->pdi, N); rows(d->pdb, q->pdb, n); rows(d->pdbi, q->pdbi, n); rows(d->pc, q->pc, 1); rows(d->pc_inv, q->pc_inv, 1);
    rows(d->rho, q->rho, 1); rows(d->delta, q->delta, 1); rows(d->trace, q->trace, (size_t)q->trace_max * 11);
    d->tab.alloc(d->tab_h.size());
    if (q->per_inst) {
        d->cnt_d.alloc(4 * B);
        kb_gather_rows(st, d->tab.p, q->tab.p, sel.dev, B, sizeof(int) * d->tab_stride());
        kb_gather_rows(st, d->cnt_d.p, q->cnt_d.p, sel.dev, B, sizeof(int) * 4);
    } else if (q->tab.n) PQ_HIP(hipMemcpyAsync(d->tab.p, q->tab.p, q->tab.bytes(), hipMemcpyDeviceToDevice, st));
    d->flags.alloc(B); d->act.alloc(2 * B); d->counters.alloc(8); d->counters_h.alloc(4);
    d->flags.zero(st); d->act.zero(st); d->counters.zero(st);
    d->dead_d.alloc(B * m); d->raw.alloc(B * n * (size_t)std::max(n, std::max(p, m))); d->bnd_h.alloc(2 * B * (2 * (size_t)m + 2 * (size_t)n));
    d->state.alloc(B); d->state_h.alloc(B);
    kb_gather_rows(st, d->state.p, q->state.p, sel.dev, B, sizeof(DsbState));
    kb_gather_host(d->state_h.p, q->state_h.p, idx, count, 1);
    PQ_HIP(hipEventRecord(d->ev[1], st));
    kb_gather_timed(sel, st, d->ev[0], d->ev[1]);
    c->clone_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    c->pr = std::move(d);
}

}  // namespace

extern "C" {

int pq_solver_batch_create(pq_solver_batch** out, int device)
{
    if (!out) return fail(PQ_ERR_INVALID, "null argument");
    if (device < 0) return fail(PQ_ERR_INVALID, "dense solver batch: device = %d", device);
    return guarded([&] {
        std::unique_ptr<pq_solver_batch> s(new pq_solver_batch);
        s->device = device;
        pq_settings_default(&s->settings);
        std::memset(&s->invalid_info, 0, sizeof(pq_info));
        s->invalid_info.status = PQ_UNSOLVED;
        *out = s.release();
        return (int)PQ_OK;
    });
}

void pq_solver_batch_destroy(pq_solver_batch* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int pq_solver_batch_clone(const pq_solver_batch* s, pq_solver_batch** out)
{
    if (!s || !out) return fail(PQ_ERR_INVALID, "null argument");
    return guarded([&] {
        std::unique_ptr<pq_solver_batch> c(dsb_clone_scalars(s));
        if (s->pr) {  // the identity list
            std::vector<int> all((size_t)s->pr->batch);
            for (size_t i = 0; i < all.size(); ++i) all[i] = (int)i;
            dsb_clone_problem(s, c.get(), all.data(), (int)all.size());
        }
        *out = c.release();
        return (int)PQ_OK;
    });
}

int pq_solver_batch_clone_select(const pq_solver_batch* s, const int* idx, int count, pq_solver_batch** out)
{
    if (!s || !out) return fail(PQ_ERR_INVALID, "null argument");
    if (int rc = kb_check_list("dense solver batch", idx, count)) return rc;
    if (!s->pr) return fail(PQ_ERR_INVALID, "dense solver batch: clone_select before setup (there is no instance to select)");
    if (int rc = kb_check_select("dense solver batch", s->pr->batch, idx, count)) return rc;
    return guarded([&] {
        std::unique_ptr<pq_solver_batch> c(dsb_clone_scalars(s));
        dsb_clone_problem(s, c.get(), idx, count);
        *out = c.release();
        return (int)PQ_OK;
    });
}

pq_settings* pq_solver_batch_settings(pq_solver_batch* s)
{
    if (!s) { fail(PQ_ERR_INVALID, "null argument"); return nullptr; }
    return &s->settings;
}

int pq_solver_batch_set_trace(pq_solver_batch* s, int max_rows)
{
    if (!s) return fail(PQ_ERR_INVALID, "null argument");
    if (max_rows < 0) return fail(PQ_ERR_INVALID, "dense solver batch: max_rows = %d is negative", max_rows);
    if (s->pr && max_rows > s->pr->trace_max)
        return fail(PQ_ERR_INVALID, "dense solver batch: the trace is sized at setup (%d rows): ask for %d rows before the setup (only setup may allocate)", s->pr->trace_max, max_rows);
    s->trace_max = max_rows;
    return PQ_OK;
}

int pq_solver_batch_set_bound_sets(pq_solver_batch* s, int mode)
{
    if (!s) return fail(PQ_ERR_INVALID, "null argument");
    if (mode != PQ_BOUND_SETS_SHARED && mode != PQ_BOUND_SETS_PER_INSTANCE)
        return fail(PQ_ERR_INVALID, "dense solver batch: bound sets %d: PQ_BOUND_SETS_SHARED or PQ_BOUND_SETS_PER_INSTANCE wanted", mode);
    s->bound_sets = mode;  // (a problem that is set up keeps the mode its setup read)
    return PQ_OK;
}

int pq_debug_bound_lists(int m, int n, const double* h_l, const double* h_u, const double* x_l, const double* x_u, const int* fin_h_l, const int* fin_h_u, const int* fin_x_l,
                         const int* fin_x_u, int counts[4], int* h_l_idx, int* h_u_idx, int* x_l_idx, int* x_u_idx, int* dead, double* h_l_out, double* h_u_out, double* x_l_out,
                         double* x_u_out)
{
    if (m < 0 || n < 1 || !counts) return fail(PQ_ERR_INVALID, "bound lists: m = %d, n = %d, counts %s: m >= 0, n >= 1 and counts wanted", m, n, counts ? "given" : "null");
    const bool any = fin_h_l || fin_h_u || fin_x_l || fin_x_u;
    if (any && ((m > 0 && (!fin_h_l || !fin_h_u)) || !fin_x_l || !fin_x_u))
        return fail(PQ_ERR_INVALID, "bound lists: the stored flags of an update are four vectors, or none for a setup");
    const int* fin[4] = {fin_h_l, fin_h_u, fin_x_l, fin_x_u};
    int* idx[4] = {h_l_idx, h_u_idx, x_l_idx, x_u_idx};
    double* packed[4] = {h_l_out, h_u_out, x_l_out, x_u_out};
    dsb_bound_lists(m, n, h_l, h_u, x_l, x_u, any ? fin : nullptr, counts, idx, dead, packed);
    return PQ_OK;
}

int pq_solver_batch_setup_dense(pq_solver_batch* s, int batch, int n, int p, int m, const double* P, const double* c, const double* A, const double* b, const double* G,
                                const double* h_l, const double* h_u, const double* x_l, const double* x_u, int mem, int order)
{
    if (!s) return fail(PQ_ERR_INVALID, "null argument");
    if (batch < 1 || n < 1 || p < 0 || m < 0)
        return fail(PQ_ERR_INVALID, "dense solver batch: batch = %d, n = %d, p = %d, m = %d: batch, n >= 1 and p, m >= 0 wanted", batch, n, p, m);
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense solver batch: bad mem %d", mem);
    if (order != PQ_COL_MAJOR && order != PQ_ROW_MAJOR) return fail(PQ_ERR_INVALID, "dense solver batch: bad order %d", order);
    const int kind = s->settings.kkt_solver;
    if (kind != PQ_DENSE_CHOLESKY && kind != PQ_DENSE_LDLT_NO_PIVOT)
        return fail(PQ_ERR_INVALID, "dense solver batch: kkt_solver = %d: PQ_DENSE_CHOLESKY or PQ_DENSE_LDLT_NO_PIVOT wanted", kind);
    if (!P || !c) return fail(PQ_ERR_INVALID, "dense solver batch: P and c must be given");
    if (p > 0 && !A) return fail(PQ_ERR_INVALID, "dense solver batch: A is null, p = %d", p);
    if (m > 0 && !G) return fail(PQ_ERR_INVALID, "dense solver batch: G is null, m = %d", m);
    if (int rc = dsb_check_refine_cap(s->settings)) return rc;
    if (n > PQ_KKT_BATCH_DENSE_MAX_N) return fail(PQ_ERR_UNSUPPORTED, "dense solver batch: n = %d, the limit is n <= %d", n, (int)PQ_KKT_BATCH_DENSE_MAX_N);
    return guarded([&] {
        PQ_HIP(hipSetDevice(s->device));
        const size_t B = (size_t)batch, N = (size_t)n + p + m;
        // the vectors on the host: the finite-bound lists are host logic (dsb_bound_lists), one set for the batch or one per instance
        auto fetch = [&](const double* src, size_t len) {
            std::vector<double> v;
            if (!src || !len) return v;
            v.resize(B * len);
            PQ_HIP(hipMemcpy(v.data(), src, sizeof(double) * v.size(), mem == PQ_MEM_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
            return v;
        };
        std::vector<double> hc = fetch(c, n), hb = fetch(b, p), hhl = fetch(h_l, m), hhu = fetch(h_u, m), hxl = fetch(x_l, n), hxu = fetch(x_u, n);
        if (hb.empty()) hb.assign(B * p, 0.0);
        std::unique_ptr<DsbProblem> q(new DsbProblem);
        q->batch = batch; q->n = n; q->p = p; q->m = m; q->trace_max = s->trace_max;
        q->per_inst = s->bound_sets == PQ_BOUND_SETS_PER_INSTANCE;
        const int R = q->rows = q->per_inst ? batch : 1;
        q->cnt_h.assign(4 * (size_t)R, 0); q->lists_h.assign((size_t)R * (2 * (size_t)m + 2 * (size_t)n), 0); q->fin_h.assign(q->lists_h.size(), 0);
        q->try_h.assign(2 * (size_t)m + 2 * (size_t)n + 4, 0); q->dead_h.assign(B * m, 0);
        if (q->per_inst) { q->keep_h.assign(q->cnt_h.size() + q->lists_h.size(), 0); q->relisted_h.assign(B, 0); }
        std::vector<double> vhl(B * m), vhu(B * m), vxl(B * n, 0.0), vxu(B * n, 0.0);
        for (size_t i = 0; i < B; ++i) {
            // the lists of instance i: its own row, or with shared sets those of instance 0, which every other instance must reproduce (with the rows it drops)
            const bool own = q->per_inst || i == 0;
            int* t = q->try_h.data();
            int* idx[4] = {own ? q->list(0, i) : t, own ? q->list(1, i) : t + m, own ? q->list(2, i) : t + 2 * (size_t)m, own ? q->list(3, i) : t + 2 * (size_t)m + n};
            int* cnt = own ? q->cnt_h.data() + 4 * i : t + 2 * (size_t)m + 2 * (size_t)n;
            double* packed[4] = {vhl.data() + i * m, vhu.data() + i * m, vxl.data() + i * n, vxu.data() + i * n};
            dsb_bound_lists(m, n, hhl.empty() ? nullptr : hhl.data() + i * m, hhu.empty() ? nullptr : hhu.data() + i * m, hxl.empty() ? nullptr : hxl.data() + i * n,
                            hxu.empty() ? nullptr : hxu.data() + i * n, nullptr, cnt, idx, q->dead_h.data() + i * m, packed);
            if (own) continue;
            bool same = std::equal(cnt, cnt + 4, q->cnt_h.data()) && std::equal(q->dead_h.begin(), q->dead_h.begin() + m, q->dead_h.begin() + i * m);
            for (int k = 0; k < 4 && same; ++k) same = std::equal(idx[k], idx[k] + cnt[k], q->list(k, 0));
            if (!same) throw std::runtime_error("dense solver batch: the set of finite bounds differs from the one of instance 0 (it is shared by the batch)");
        }
        q->tab_h.assign((size_t)R * q->tab_stride(), -1);
        q->fill_tab();
        q->fill_fin();
        // the matrices: upper(P), A', G' column-major in temporaries, equilibrated there, then handed to the KKT system (which keeps its own copies)
        Stream st(s->device);
        DBuf<double> Pu(B * n * n), AT(B * n * p), GT(B * n * m);
        q->tab.alloc(q->tab_h.size());
        if (q->per_inst) q->cnt_d.alloc(4 * B);
        q->dead_d.alloc(B * m); q->raw.alloc(B * n * (size_t)std::max(n, std::max(p, m))); q->bnd_h.alloc(2 * B * (2 * (size_t)m + 2 * (size_t)n));
        if (!q->tab_h.empty()) PQ_HIP(hipMemcpyAsync(q->tab.p, q->tab_h.data(), sizeof(int) * q->tab_h.size(), hipMemcpyHostToDevice, st));
        if (q->per_inst) PQ_HIP(hipMemcpyAsync(q->cnt_d.p, q->cnt_h.data(), sizeof(int) * 4 * B, hipMemcpyHostToDevice, st));
        const int dead_stride = q->per_inst ? m : 0;  // (shared sets: every instance drops the rows instance 0 drops)
        if (m > 0) PQ_HIP(hipMemcpyAsync(q->dead_d.p, q->dead_h.data(), sizeof(int) * (size_t)R * m, hipMemcpyHostToDevice, st));
        const DsbRows all{nullptr, nullptr, batch};
        dsb_matrix(q.get(), st, all, P, Pu.p, n, order == PQ_COL_MAJOR ? 2 : 3, nullptr, 0, mem);
        dsb_matrix(q.get(), st, all, A, AT.p, p, order == PQ_COL_MAJOR ? 1 : 0, nullptr, 0, mem);
        dsb_matrix(q.get(), st, all, G, GT.p, m, order == PQ_COL_MAJOR ? 1 : 0, q->dead_d.p, dead_stride, mem);
        auto up = [&](DBuf<double>& d, const std::vector<double>& v, size_t count) {
            d.alloc(count);
            if (count) PQ_HIP(hipMemcpyAsync(d.p, v.data(), sizeof(double) * count, hipMemcpyHostToDevice, st));
        };
        const std::vector<double> ones(B * n, 1.0);
        up(q->c, hc, B * n); up(q->b, hb, B * p); up(q->h_l, vhl, B * m); up(q->h_u, vhu, B * m); up(q->x_l, vxl, B * n); up(q->x_u, vxu, B * n); up(q->xbs, ones, B * n);
        q->pd.alloc(B * N); q->pdi.alloc(B * N); q->pdb.alloc(B * n); q->pdbi.alloc(B * n); q->pc.alloc(B); q->pc_inv.alloc(B);
        dsb_launch_ruiz(s, q.get(), st, all, Pu.p, AT.p, GT.p, 0);
        stream_wait(st);
        pq_kktsys_batch* ks = nullptr;
        const int* cn = q->cnt_h.data();
        if (int rc = q->per_inst ? pq_kktsys_batch_create_dense_lists(&ks, s->device, batch, n, p, m, Pu.p, AT.p, GT.p, cn, q->list(0, 0), q->list(1, 0), q->list(2, 0), q->list(3, 0),
                                                                      q->xbs.p, &s->settings, PQ_MEM_DEVICE)
                                 : pq_kktsys_batch_create_dense(&ks, s->device, batch, n, p, m, Pu.p, AT.p, GT.p, cn[0], cn[1], cn[2], cn[3], q->list(0, 0), q->list(1, 0), q->list(2, 0),
                                                                q->list(3, 0), q->xbs.p, &s->settings, PQ_MEM_DEVICE))
            return rc;
        q->ks.reset(ks);
        hipStream_t kst = ksb_stream(ks);
        for (VarSet& v : q->sets) v.alloc(B, n, p, m, kst);
        q->rho.alloc(B); q->delta.alloc(B); q->flags.alloc(B); q->act.alloc(2 * B); q->counters.alloc(8); q->counters_h.alloc(4);
        q->flags.zero(kst); q->act.zero(kst); q->counters.zero(kst);
        q->trace.alloc(B * (size_t)q->trace_max * 11);
        q->trace.zero(kst);
        q->state.alloc(B); q->state_h.alloc(B);
        for (Event& e : q->ev) e = Event(0);
        s->pr = std::move(q);
        dsb_reset_state(s);  // init_workspace :361-377
        PQ_HIP(hipMemcpyAsync(s->pr->state.p, s->pr->state_h.p, sizeof(DsbState) * B, hipMemcpyHostToDevice, kst));
        stream_wait(kst);
        s->solved = false;
        s->updated = false;
        return 1;
    });
}

// ---- update: pq_solver_batch_update_dense (idx = null: row j of every array is instance j, `count` is the batch) and pq_solver_batch_update_dense_select (row j is
// instance idx[j]; the list has been checked) are this one sequence.  Everything of the call goes by its ROWS: the fetched and the packed bound vectors, the mask of
// the rows of G it drops (dead_h, dead_d); what is kept per instance -- lists, tables, data -- is reached through the row's instance.  With a list every launch is
// sized by it and no workgroup runs on an instance that is not listed.
static int dsb_update(pq_solver_batch* s, const int* idx, int count, const double* P, const double* c, const double* A, const double* b, const double* G, const double* h_l,
                      const double* h_u, const double* x_l, const double* x_u, int mem, int order)
{
    DsbProblem* q = s->pr.get();
    return guarded([&] {
        PQ_HIP(hipSetDevice(s->device));
        const auto w0 = std::chrono::steady_clock::now();
        const int batch = q->batch, n = q->n, p = q->p, m = q->m;
        const size_t B = (size_t)batch, R = (size_t)count, half = B * (2 * (size_t)m + 2 * (size_t)n);
        pq_kktsys_batch* ks = q->ks.get();
        pq_kkt_batch* kb = pq_kktsys_batch_backend(ks);
        hipStream_t st = ksb_stream(ks);
        DsbRows rw{idx, nullptr, count};  // (the list goes up behind the host's checks: a refused call has done nothing on the device and allocated nothing)
        // ---- the host: the lists the reference would hold after this call (dsb_bound_lists): with shared sets they must be the setup's, else they replace the instance's own
        const double* given[4] = {h_l, h_u, x_l, x_u};
        const double* hv[4];
        double* packed[4];
        bool fetched = false;
        for (int k = 0; k < 4; ++k) {
            const size_t off = k == 0 ? 0 : k == 1 ? B * m : k == 2 ? 2 * B * m : 2 * B * m + B * n, cnt = R * (k < 2 ? m : n);
            packed[k] = q->bnd_h.p + half + off;
            hv[k] = given[k];
            if (given[k] && mem == PQ_MEM_DEVICE && cnt) {
                PQ_HIP(hipMemcpyAsync(q->bnd_h.p + off, given[k], sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
                hv[k] = q->bnd_h.p + off;
                fetched = true;
            }
        }
        if (fetched) stream_wait(st);
        const bool rows = h_l || h_u;
        // sets per instance: the host images of the call's instances are rewritten below, before the device and the KKT system follow.  Should a call on the way fail,
        // those rows go back to what the device still holds (a failure after the new tables are on their way leaves the device ahead of the host: then only a new
        // setup helps).  Only what the call touches is kept and put back.
        struct Keep {
            DsbProblem* q;
            const DsbRows& rw;
            bool done = false;
            void move(bool back)
            {
                int* kc = q->keep_h.data();
                int* kl = kc + q->cnt_h.size();
                for (int j = 0; j < rw.count; ++j) {
                    const size_t i = (size_t)rw.inst(j);
                    int* a = q->cnt_h.data() + 4 * i;
                    if (back) std::copy(kc + 4 * i, kc + 4 * i + 4, a);
                    else std::copy(a, a + 4, kc + 4 * i);
                    for (int k = 0; k < 4; ++k) {
                        int* l = q->list(k, i);
                        int* kp = kl + (l - q->lists_h.data());
                        const int len = k < 2 ? q->m : q->n;
                        if (back) std::copy(kp, kp + len, l);
                        else std::copy(l, l + len, kp);
                    }
                }
            }
            Keep(DsbProblem* p, const DsbRows& r) : q(p), rw(r)
            {
                if (q->per_inst) move(false);
            }
            ~Keep()
            {
                if (done || !q->per_inst) return;
                move(true);
                q->fill_fin();
                q->fill_tab();
            }
        } keep(q, rw);
        bool any_dead = false;
        for (size_t j = 0; j < R; ++j) {
            const size_t i = (size_t)rw.inst((int)j), r = q->per_inst ? i : 0;
            const int* fin[4] = {q->fin(0, r), q->fin(1, r), q->fin(2, r), q->fin(3, r)};
            int* t = q->try_h.data();
            int* lst[4] = {q->per_inst ? q->list(0, i) : t, q->per_inst ? q->list(1, i) : t + m, q->per_inst ? q->list(2, i) : t + 2 * (size_t)m,
                           q->per_inst ? q->list(3, i) : t + 2 * (size_t)m + n};
            int* cnt = q->per_inst ? q->cnt_h.data() + 4 * i : t + 2 * (size_t)m + 2 * (size_t)n;
            double* out[4] = {packed[0] + j * m, packed[1] + j * m, packed[2] + j * n, packed[3] + j * n};
            dsb_bound_lists(m, n, h_l ? hv[0] + j * m : nullptr, h_u ? hv[1] + j * m : nullptr, x_l ? hv[2] + j * n : nullptr, x_u ? hv[3] + j * n : nullptr, fin, cnt, lst,
                            q->dead_h.data() + j * m, out);
            for (int e = 0; e < m && rows && !any_dead; ++e) any_dead = q->dead_h[j * m + e] != 0;
            if (q->per_inst) continue;
            for (int k = 0; k < 4; ++k) {  // shared sets: the lists are the setup's, which the KKT system and `tab` carry
                const int* old = q->list(k, 0);
                const int co = q->cnt_h[k];
                int e = 0;
                while (e < cnt[k] && e < co && lst[k][e] == old[e]) ++e;
                if (e == cnt[k] && e == co) continue;
                const int at = e == cnt[k] ? old[e] : e == co ? lst[k][e] : std::min(lst[k][e], old[e]);
                return fail(PQ_ERR_INVALID, "dense solver batch: update: the set of finite bounds of %s %d%s changes in instance %zu (it is fixed at setup)", k < 2 ? "row" : "variable", at,
                            k < 2 ? " of G" : "", i);
            }
        }
        if (q->per_inst) {
            q->fill_fin(); q->fill_tab();
            for (int j = 0; j < count; ++j) q->relisted_h[rw.inst(j)] = 1;
        }
        // ---- the device: unscale, assign, rescale, all where the data stand
        if (idx) rw = dsb_rows_select(q, st, idx, count);
        PQ_HIP(hipEventRecord(q->ev[0], st));
        const int* dd = nullptr;
        if (any_dead) {
            PQ_HIP(hipMemcpyAsync(q->dead_d.p, q->dead_h.data(), sizeof(int) * R * m, hipMemcpyHostToDevice, st));
            dd = q->dead_d.p;
        }
        DsbUnscaleArgs u;
        u.n = n; u.p = p; u.m = m; u.list = rw.dev; u.bd = q->bounds();  // (the device still holds the tables of before this call)
        u.Pu = kb->Pu.p; u.AT = kb->AT.p; u.GT = kb->GT.p; u.c = q->c.p; u.b = q->b.p; u.h_l = q->h_l.p; u.h_u = q->h_u.p; u.x_l = q->x_l.p; u.x_u = q->x_u.p; u.xbs = q->xbs.p;
        u.pdi = q->pdi.p; u.pdbi = q->pdbi.p; u.pc_inv = q->pc_inv.p; u.dead = dd;
        if (q->per_inst) k_dsb_unscale<true><<<count, DSB_RUIZ_T, 0, st>>>(u);
        else k_dsb_unscale<false><<<count, DSB_RUIZ_T, 0, st>>>(u);
        PQ_HIP(hipGetLastError());
        if (q->per_inst) {  // the sets of after this call: the tables here (behind the unscaling on the stream) and the KKT system's.  (The whole host images go up:
                            // the rows of the instances the call does not act on are the bytes the device holds already)
            PQ_HIP(hipMemcpyAsync(q->tab.p, q->tab_h.data(), sizeof(int) * q->tab_h.size(), hipMemcpyHostToDevice, st));
            PQ_HIP(hipMemcpyAsync(q->cnt_d.p, q->cnt_h.data(), sizeof(int) * 4 * B, hipMemcpyHostToDevice, st));
            if (int rc = pq_kktsys_batch_set_lists(ks, q->cnt_h.data(), q->list(0, 0), q->list(1, 0), q->list(2, 0), q->list(3, 0))) return rc;
        }
        int opt = PQ_KKT_UPDATE_NONE;
        if (P) { dsb_matrix(q, st, rw, P, kb->Pu.p, n, order == PQ_COL_MAJOR ? 2 : 3, nullptr, 0, mem); opt |= PQ_KKT_UPDATE_P; }
        if (A) { dsb_matrix(q, st, rw, A, kb->AT.p, p, order == PQ_COL_MAJOR ? 1 : 0, nullptr, 0, mem); opt |= PQ_KKT_UPDATE_A; }
        if (G) { dsb_matrix(q, st, rw, G, kb->GT.p, m, order == PQ_COL_MAJOR ? 1 : 0, dd, m, mem); opt |= PQ_KKT_UPDATE_G; }
        if (c) dsb_vector(q, st, rw, c, q->c.p, (size_t)n, mem);
        if (b) dsb_vector(q, st, rw, b, q->b.p, (size_t)p, mem);
        DBuf<double>* dst[4] = {&q->h_l, &q->h_u, &q->x_l, &q->x_u};
        for (int k = 0; k < 4; ++k)
            if (given[k]) dsb_vector(q, st, rw, packed[k], dst[k]->p, (size_t)(k < 2 ? m : n), PQ_MEM_HOST);
        const bool reuse = s->settings.preconditioner_reuse_on_update || opt == PQ_KKT_UPDATE_NONE;
        dsb_launch_ruiz(s, q, st, rw, kb->Pu.p, kb->AT.p, kb->GT.p, reuse);
        // A'A: the reference takes it again only with A; with new scalings it has to follow A' (the header says why)
        ksb_data_rewritten(ks, opt, A != nullptr || !reuse, q->xbs.p, rw.dev, count);
        PQ_HIP(hipEventRecord(q->ev[1], st));
        stream_wait(st);
        float ms = 0.f;
        PQ_HIP(hipEventElapsedTime(&ms, q->ev[0], q->ev[1]));
        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        for (int j = 0; j < count; ++j) q->state_h.p[rw.inst(j)].info.update_time = wall * 1e-3;  // (the call's)
        s->update_wall_ms = wall; s->update_device_ms = ms;
        s->updated = true;
        keep.done = true;
        return 1;
    });
}

int pq_solver_batch_update_dense(pq_solver_batch* s, const double* P, const double* c, const double* A, const double* b, const double* G, const double* h_l,
                                 const double* h_u, const double* x_l, const double* x_u, int mem, int order)
{
    if (!s) return fail(PQ_ERR_INVALID, "null argument");
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense solver batch: bad mem %d", mem);
    if (order != PQ_COL_MAJOR && order != PQ_ROW_MAJOR) return fail(PQ_ERR_INVALID, "dense solver batch: bad order %d", order);
    DsbProblem* q = s->pr.get();
    if (!q) return fail(PQ_ERR_INVALID, "dense solver batch: update before setup");
    if (q->p == 0 && (A || b)) return fail(PQ_ERR_INVALID, "dense solver batch: update: A or b given, p = 0");
    if (q->m == 0 && (G || h_l || h_u)) return fail(PQ_ERR_INVALID, "dense solver batch: update: G, h_l or h_u given, m = 0");
    return dsb_update(s, nullptr, q->batch, P, c, A, b, G, h_l, h_u, x_l, x_u, mem, order);
}

int pq_solver_batch_update_dense_select(pq_solver_batch* s, const int* idx, int count, const double* P, const double* c, const double* A, const double* b, const double* G,
                                        const double* h_l, const double* h_u, const double* x_l, const double* x_u, int mem, int order)
{
    static const char* const fn = "pq_solver_batch_update_dense_select";
    if (int rc = dsb_check_list(fn, s, idx, count)) return rc;
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "%s: bad mem %d", fn, mem);
    if (order != PQ_COL_MAJOR && order != PQ_ROW_MAJOR) return fail(PQ_ERR_INVALID, "%s: bad order %d", fn, order);
    if (int rc = dsb_check_entries(fn, s, idx, count, true)) return rc;
    const DsbProblem* q = s->pr.get();
    if (q->p == 0 && (A || b)) return fail(PQ_ERR_INVALID, "%s: A or b given, p = 0", fn);
    if (q->m == 0 && (G || h_l || h_u)) return fail(PQ_ERR_INVALID, "%s: G, h_l or h_u given, m = 0", fn);
    return dsb_update(s, idx, count, P, c, A, b, G, h_l, h_u, x_l, x_u, mem, order);
}

int pq_solver_batch_last_update_ms(const pq_solver_batch* s, double out2[2])
{
    if (!s || !out2) return fail(PQ_ERR_INVALID, "null argument");
    out2[0] = s->update_wall_ms; out2[1] = s->update_device_ms;
    return PQ_OK;
}

// ---- solve: pq_solver_batch_solve (idx = null, `count` is the batch) and pq_solver_batch_solve_select (the `count` distinct instances idx[..], checked) are this
// one loop.  With a list every launch has one workgroup (in the packed factor kernel one wave) per listed instance, the round loop ends when the DONE counter
// reaches count, and only the listed infos are written on the host.  The state records travel whole in both forms: the host image goes up before the first round and
// comes back after the last -- between the two no workgroup has touched the record of an instance that is not listed, so its host record gets its own bytes back.
static int dsb_solve(pq_solver_batch* s, const int* idx, int count)
{
    DsbProblem* q = s->pr.get();
    const DsbRows on_host{idx, nullptr, count};
    if (int rc = dsb_check_refine_cap(s->settings)) return rc;
    if (!dsb_verify_settings(s->settings)) {  // solver.hpp:75-79: no launch
        for (int j = 0; j < count; ++j) q->state_h.p[on_host.inst(j)].info.status = PQ_INVALID_SETTINGS;
        return fail(PQ_ERR_INVALID, "dense solver batch: invalid settings");
    }
    int solved = 0, rc_loop = PQ_OK;
    const int rc = guarded([&] {
        PQ_HIP(hipSetDevice(s->device));
        const auto w0 = std::chrono::steady_clock::now();
        const int batch = q->batch, n = q->n, p = q->p, m = q->m;
        pq_kktsys_batch* ks = q->ks.get();
        {
            pq_settings ks_set = s->settings;
            if (int e = pq_kktsys_batch_set_settings(ks, &ks_set)) return e;
        }
        hipStream_t st = ksb_stream(ks);
        pq_kkt_batch* kb = pq_kktsys_batch_backend(ks);
        const DsbRows rw = idx ? dsb_rows_select(q, st, idx, count) : DsbRows{nullptr, nullptr, batch};
        // every instance of the call starts at INIT (the info fields a solve does not reset keep their values)
        for (int j = 0; j < count; ++j) q->state_h.p[rw.inst(j)].stage = ST_INIT;
        PQ_HIP(hipMemcpyAsync(q->state.p, q->state_h.p, sizeof(DsbState) * batch, hipMemcpyHostToDevice, st));
        PQ_HIP(hipMemsetAsync(q->counters.p, 0, sizeof(int) * 8, st));
        DsbArgs a;
        a.n = n; a.p = p; a.m = m; a.bd = q->bounds(); a.batch = batch; a.trace_max = q->trace_max; a.slot = 0; a.list = rw.dev;
        a.set = s->settings;
        a.Pu = kb->Pu.p; a.AT = kb->AT.p; a.GT = kb->GT.p;
        a.c = q->c.p; a.b = q->b.p; a.h_l = q->h_l.p; a.h_u = q->h_u.p; a.x_l = q->x_l.p; a.x_u = q->x_u.p; a.xbs = q->xbs.p;
        a.pd = q->pd.p; a.pdb = q->pdb.p; a.pdi = q->pdi.p; a.pdbi = q->pdbi.p; a.pc_inv = q->pc_inv.p;
        a.r = q->sets[0].v; a.nr = q->sets[1].v; a.res = q->sets[2].v; a.st = q->sets[3].v; a.px = q->sets[4].v;
        a.state = q->state.p; a.rho = q->rho.p; a.delta = q->delta.p; a.flags = q->flags.p; a.act_f = q->act.p; a.act_s = q->act.p + batch; a.counters = q->counters.p;
        a.fstatus = ksb_factor_status(ks); a.sinfo = ksb_solve_info(ks);
        a.trace = q->trace_max > 0 ? q->trace.p : nullptr;
        // one instance needs at most max_iter + 1 passes of the loop, each at most max_factor_retires + 2 factor rounds and 2 solve rounds
        const long long bound = ((long long)s->settings.max_iter + 1) * ((long long)s->settings.max_factor_retires + 4);
        long long round = 0;
        int launches = 0;
        double dev_ms = 0.0, f_ms = 0.0, s_ms = 0.0;
        bool pend_f = false, pend_s = false, done = false;
        auto elapsed = [&](int e) {
            float ms = 0.f;
            PQ_HIP(hipEventElapsedTime(&ms, q->ev[e], q->ev[e + 1]));
            return (double)ms;
        };
        for (; round < bound && !done; ++round) {
            a.slot = (int)(round & 1);
            PQ_HIP(hipEventRecord(q->ev[0], st));
            if (q->per_inst) {
                if (rw.dev) k_dsb_advance<true, true><<<count, DSB_T, 0, st>>>(a);
                else k_dsb_advance<true, false><<<count, DSB_T, 0, st>>>(a);
            } else if (rw.dev) k_dsb_advance<false, true><<<count, DSB_T, 0, st>>>(a);
            else k_dsb_advance<false, false><<<count, DSB_T, 0, st>>>(a);
            PQ_HIP(hipGetLastError());
            PQ_HIP(hipEventRecord(q->ev[1], st));
            PQ_HIP(hipMemcpyAsync(q->counters_h.p, q->counters.p + 4 * a.slot, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
            stream_wait(st);
            ++launches;
            dev_ms += elapsed(0);
            if (pend_f) { const double t = elapsed(2); dev_ms += t; f_ms += t; pend_f = false; }
            if (pend_s) { const double t = elapsed(4); dev_ms += t; s_ms += t; pend_s = false; }
            const int nf = q->counters_h.p[WANT_FACTOR], ns = q->counters_h.p[WANT_SOLVE], nd = q->counters_h.p[WANT_DONE];
            if (nd == count) { done = true; continue; }
            if (nf > 0) {
                PQ_HIP(hipEventRecord(q->ev[2], st));
                // (a factor launch over the whole batch ends the KKT system's `stale` state after pq_kktsys_batch_set_lists: right here, because after an update every
                // instance starts at INIT and the first round's launch factors them all; one over a list leaves it to the end of this call)
                ksb_launch_factor(ks, q->flags.p, q->rho.p, q->delta.p, q->sets[0].v, a.act_f, rw.dev, count);
                PQ_HIP(hipEventRecord(q->ev[3], st));
                pend_f = true;
                ++launches;
            }
            if (ns > 0) {
                PQ_HIP(hipEventRecord(q->ev[4], st));
                ksb_launch_solve(ks, q->sets[2].v, q->sets[3].v, a.act_s, rw.dev, count);
                PQ_HIP(hipEventRecord(q->ev[5], st));
                pend_s = true;
                ++launches;
            }
        }
        DsbFinishArgs f;
        f.n = n; f.p = p; f.m = m; f.list = rw.dev; f.bd = q->bounds();
        f.pd = q->pd.p; f.pdb = q->pdb.p; f.pdi = q->pdi.p; f.pdbi = q->pdbi.p; f.pc_inv = q->pc_inv.p;
        f.r = q->sets[0].v; f.out = q->sets[5].v;
        PQ_HIP(hipEventRecord(q->ev[6], st));
        if (q->per_inst) k_dsb_finish<true><<<count, DSB_T, 0, st>>>(f);
        else k_dsb_finish<false><<<count, DSB_T, 0, st>>>(f);
        PQ_HIP(hipGetLastError());
        PQ_HIP(hipEventRecord(q->ev[7], st));
        ++launches;
        PQ_HIP(hipMemcpyAsync(q->state_h.p, q->state.p, sizeof(DsbState) * batch, hipMemcpyDeviceToHost, st));
        ksb_refresh_host(ks);  // (waits)
        if (pend_f) { const double t = elapsed(2); dev_ms += t; f_ms += t; }
        if (pend_s) { const double t = elapsed(4); dev_ms += t; s_ms += t; }
        dev_ms += elapsed(6);
        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        for (int j = 0; j < count; ++j) {
            DsbState& S = q->state_h.p[rw.inst(j)];
            pq_info& I = S.info;
            if (!done && S.stage != ST_DONE) I.status = PQ_UNSOLVED;
            solved += I.status == PQ_SOLVED;
            I.solve_time = wall * 1e-3;  // (the call's)
            I.run_time = (s->updated ? I.update_time : I.setup_time) + I.solve_time;
        }
        if (q->per_inst) {  // every instance of the call was factored in the first round; the KKT system's lists are all in use again once no other one waits
            for (int j = 0; j < count; ++j) q->relisted_h[rw.inst(j)] = 0;
            if (round > 0 && std::find(q->relisted_h.begin(), q->relisted_h.end(), (char)1) == q->relisted_h.end()) ksb_lists_factored(ks);
        }
        s->wall_ms = wall; s->device_ms = dev_ms; s->factor_ms = f_ms; s->solve_ms = s_ms; s->rounds = (int)round; s->launches = launches;
        s->solved = true;
        if (!done) rc_loop = fail(PQ_ERR_INTERNAL, "dense solver batch: %lld rounds (the bound) did not finish every instance", bound);
        return (int)PQ_OK;
    });
    if (rc != PQ_OK) return rc;
    return rc_loop != PQ_OK ? rc_loop : solved;
}

int pq_solver_batch_solve(pq_solver_batch* s)
{
    if (!s) return fail(PQ_ERR_INVALID, "null argument");
    if (!s->pr) {
        s->invalid_info.status = PQ_UNSOLVED;
        return fail(PQ_ERR_INVALID, "dense solver batch: solve before setup");
    }
    return dsb_solve(s, nullptr, s->pr->batch);
}

int pq_solver_batch_solve_select(pq_solver_batch* s, const int* idx, int count)
{
    static const char* const fn = "pq_solver_batch_solve_select";
    if (int rc = dsb_check_list(fn, s, idx, count)) return rc;
    if (int rc = dsb_check_entries(fn, s, idx, count, true)) return rc;
    return dsb_solve(s, idx, count);
}

const pq_info* pq_solver_batch_info(const pq_solver_batch* s, int instance)
{
    if (!s) { fail(PQ_ERR_INVALID, "null argument"); return nullptr; }
    if (!s->pr) return &s->invalid_info;
    if (instance < 0 || instance >= s->pr->batch) { fail(PQ_ERR_INVALID, "dense solver batch: instance %d outside [0, %d)", instance, s->pr->batch); return nullptr; }
    return &s->pr->state_h.p[instance].info;
}

int pq_solver_batch_get_result_mem(pq_solver_batch* s, int field, double* out, int mem)
{
    if (!s || !out) return fail(PQ_ERR_INVALID, "null argument");
    if (field < 0 || field > 9) return fail(PQ_ERR_INVALID, "dense solver batch: field %d: 0 .. 9 wanted", field);
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "dense solver batch: bad mem %d", mem);
    if (!s->pr || !s->solved) return fail(PQ_ERR_INVALID, "dense solver batch: no solve yet");
    return guarded([&] {
        PQ_HIP(hipSetDevice(s->device));
        DsbProblem* q = s->pr.get();
        const size_t count = (size_t)q->batch * dsb_field_len(q, field);
        hipStream_t st = ksb_stream(q->ks.get());
        if (count) PQ_HIP(hipMemcpyAsync(out, (&q->sets[5].v.x)[field], sizeof(double) * count, mem == PQ_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        stream_wait(st);
        return (int)PQ_OK;
    });
}

int pq_solver_batch_get_result_select_mem(pq_solver_batch* s, const int* idx, int count, int field, double* out, int mem)
{
    static const char* const fn = "pq_solver_batch_get_result_select_mem";
    if (int rc = dsb_check_list(fn, s, idx, count)) return rc;
    if (!out) return fail(PQ_ERR_INVALID, "%s: out is null", fn);
    if (field < 0 || field > 9) return fail(PQ_ERR_INVALID, "%s: field %d: 0 .. 9 wanted", fn, field);
    if (kb_bad_mem(mem)) return fail(PQ_ERR_INVALID, "%s: bad mem %d", fn, mem);
    if (int rc = dsb_check_entries(fn, s, idx, count, false)) return rc;
    if (!s->solved) return fail(PQ_ERR_INVALID, "%s: no solve yet", fn);
    return guarded([&] {
        PQ_HIP(hipSetDevice(s->device));
        DsbProblem* q = s->pr.get();
        const size_t len = dsb_field_len(q, field);
        if (!len) return (int)PQ_OK;
        hipStream_t st = ksb_stream(q->ks.get());
        DBuf<double> stage;  // a host out: [count][len] on the device first
        if (mem == PQ_MEM_HOST) stage.alloc((size_t)count * len);
        double* to = mem == PQ_MEM_HOST ? stage.p : out;
        const double* from = (&q->sets[5].v.x)[field];
        for (int j0 = 0; j0 < count; j0 += q->batch) {  // (the list's buffer holds `batch` entries: a longer list goes up in pieces, each read by its gather before the next)
            const int part = std::min(q->batch, count - j0);
            const DsbRows rw = dsb_rows_select(q, st, idx + j0, part);
            kb_gather_rows(st, to + (size_t)j0 * len, from, rw.dev, (size_t)part, sizeof(double) * len);
        }
        if (mem == PQ_MEM_HOST) PQ_HIP(hipMemcpyAsync(out, stage.p, sizeof(double) * (size_t)count * len, hipMemcpyDeviceToHost, st));
        stream_wait(st);
        return (int)PQ_OK;
    });
}

int pq_solver_batch_get_trace(pq_solver_batch* s, int instance, double* out_host, int* rows_out)
{
    if (!s || !rows_out) return fail(PQ_ERR_INVALID, "null argument");
    if (!s->pr || !s->solved) return fail(PQ_ERR_INVALID, "dense solver batch: no solve yet");
    DsbProblem* q = s->pr.get();
    if (instance < 0 || instance >= q->batch) return fail(PQ_ERR_INVALID, "dense solver batch: instance %d outside [0, %d)", instance, q->batch);
    const int rows = q->state_h.p[instance].trace_rows;
    *rows_out = rows;
    if (!out_host || rows == 0) return PQ_OK;
    return guarded([&] {
        PQ_HIP(hipSetDevice(s->device));
        hipStream_t st = ksb_stream(q->ks.get());
        PQ_HIP(hipMemcpyAsync(out_host, q->trace.p + (size_t)instance * q->trace_max * 11, sizeof(double) * 11 * rows, hipMemcpyDeviceToHost, st));
        stream_wait(st);
        return (int)PQ_OK;
    });
}

int pq_solver_batch_dims(const pq_solver_batch* s, int* batch, int* n, int* p, int* m)
{
    if (!s) return fail(PQ_ERR_INVALID, "null argument");
    if (!s->pr) return fail(PQ_ERR_INVALID, "dense solver batch: no setup yet");
    if (batch) *batch = s->pr->batch;
    if (n) *n = s->pr->n;
    if (p) *p = s->pr->p;
    if (m) *m = s->pr->m;
    return PQ_OK;
}

int pq_solver_batch_clone_ms(const pq_solver_batch* s, double out2[2])
{
    if (!s || !out2) return fail(PQ_ERR_INVALID, "null argument");
    out2[0] = s->clone_wall_ms; out2[1] = s->clone_device_ms;
    return PQ_OK;
}

int pq_solver_batch_last_ms(const pq_solver_batch* s, double out6[6])
{
    if (!s || !out6) return fail(PQ_ERR_INVALID, "null argument");
    out6[0] = s->wall_ms; out6[1] = s->device_ms; out6[2] = s->rounds; out6[3] = s->launches; out6[4] = s->factor_ms; out6[5] = s->solve_ms;
    return PQ_OK;
}

int pq_solver_batch_scaled_data(pq_solver_batch* s, int instance, int what, double* out_host)
{
    if (!s || !out_host) return fail(PQ_ERR_INVALID, "null argument");
    if (!s->pr) return fail(PQ_ERR_INVALID, "dense solver batch: no setup yet");
    DsbProblem* q = s->pr.get();
    if (instance < 0 || instance >= q->batch) return fail(PQ_ERR_INVALID, "dense solver batch: instance %d outside [0, %d)", instance, q->batch);
    if (what < PQ_SOLVER_BATCH_P_UTRI || what > PQ_SOLVER_BATCH_PRECOND_C) return fail(PQ_ERR_INVALID, "dense solver batch: scaled data %d: 0 .. 12 wanted", what);
    return guarded([&] {
        PQ_HIP(hipSetDevice(s->device));
        pq_kkt_batch* kb = pq_kktsys_batch_backend(q->ks.get());
        const size_t n = q->n, p = q->p, m = q->m;
        const double* base[13] = {kb->Pu.p, kb->AT.p, kb->GT.p, q->c.p, q->b.p, q->h_l.p, q->h_u.p, q->x_l.p, q->x_u.p, q->xbs.p, q->pd.p, q->pdb.p, q->pc.p};
        const size_t len[13] = {n * n, n * p, n * m, n, p, m, m, n, n, n, n + p + m, n, 1};
        hipStream_t st = ksb_stream(q->ks.get());
        if (len[what]) PQ_HIP(hipMemcpyAsync(out_host, base[what] + (size_t)instance * len[what], sizeof(double) * len[what], hipMemcpyDeviceToHost, st));
        stream_wait(st);
        return (int)PQ_OK;
    });
}

pq_kktsys_batch* pq_solver_batch_kktsys(pq_solver_batch* s)
{
    if (!s) { fail(PQ_ERR_INVALID, "null argument"); return nullptr; }
    if (!s->pr) { fail(PQ_ERR_INVALID, "dense solver batch: no setup yet"); return nullptr; }
    return s->pr->ks.get();
}

}  // extern "C"
