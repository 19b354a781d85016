// The dual-form LP Newton steps: IPM_SOLVE_CHOLESKY_DUAL, its phase-1 form and its
// form with equality rows.  For an LP barrier H = diag(D) + C^T diag(w) C, so with E = 1 / D the step comes
// from K = diag([1 / w; 0]) + M diag(E) M^T, M = C or [C; A], of the order of the constraint rows: no n x n
// array.  All three methods share one sequence -- assemble K (syrk_nt_lower2), send the right-hand side
// through the bordered Cholesky, one backward solve, then rounds of iterative refinement on the residual of
// the full system with H applied through C, each solved on the factor -- which the file-local core below
// states once; what differs is the elementwise kernels, phase 1's second column and the A rows.
// IPM_SOLVE_CHOLESKY_DUAL_QP is the same step for a QP whose P = diag(Pdiag) + Pf^T Pf comes
// through its factors: M = [C; Pf], weights [w; t], D = t Pdiag + the bound terms; P is never formed.
// IPM_SOLVE_CHOLESKY_DUAL_QP_EQ adds the equality rows to that: M = [C; Pf; A], three
// row-stacked operands (syrk_nt_lower3, gemv_n3, gemv_t3), weights [w; t; 1], the diagonal's tail 0.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ipm_dual.h"
#include "ipm_problem.h"
#include "ipm_syrk_nt.h"

namespace ipm {
namespace {

__global__ void k_dual_combine(int64_t n, const double* __restrict__ E, const double* __restrict__ g,
                               const double* __restrict__ ctz, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = E[i] * (-g[i] - ctz[i]);
}

__global__ void k_dual_residual(int64_t n, const double* __restrict__ g, const double* __restrict__ dvec,
                                const double* __restrict__ dx, const double* __restrict__ hc,
                                double* __restrict__ rho) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) rho[i] = -g[i] - (dvec[i] * dx[i] + hc[i]);
}

__global__ void k_dual_correct(int64_t n, const double* __restrict__ E, const double* __restrict__ rho,
                               const double* __restrict__ ctz, double* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dx[i] = dx[i] + E[i] * (rho[i] - ctz[i]);
}

// ---- the dual-form QP step on a factored P (IPM_SOLVE_CHOLESKY_DUAL_QP)
// D = dvec + t Pdiag (Pdiag null: D = dvec), E = 1 / D
__global__ void k_dual_qp_diag(int64_t n, const double* __restrict__ dvec, const double* __restrict__ pdiag, double t,
                               double* __restrict__ D, double* __restrict__ E) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const double v = pdiag ? dvec[i] + t * pdiag[i] : dvec[i];
    D[i] = v;
    E[i] = 1.0 / v;
  }
}

// out = Pdiag o x + ftfx (either may be null)
__global__ void k_pfactor_combine(int64_t n, const double* __restrict__ pdiag, const double* __restrict__ x,
                                  const double* ftfx, double* out) {   // (ftfx may be out)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    double v = pdiag ? pdiag[i] * x[i] : 0.0;
    if (ftfx) v = v + ftfx[i];
    out[i] = v;
  }
}

// ---- the dual-form step with equality rows (IPM_SOLVE_CHOLESKY_DUAL_EQ): K [z; nu] = r over M = [C; A]
// r[i] = r[i] - (-axb[i] - adx[i]) = A (E o rho_x) - rho_p with rho_p = -(A x - b) - A dx (adx null: dx = 0)
__global__ void k_dual_eq_rhs(int64_t p, const double* __restrict__ axb, const double* __restrict__ adx,
                              double* __restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < p) r[i] = r[i] - (-axb[i] - (adx ? adx[i] : 0.0));
}

__global__ void k_dual_eq_combine(int64_t n, const double* __restrict__ E, const double* __restrict__ g,
                                  const double* __restrict__ ctz, const double* __restrict__ atv,
                                  double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = E[i] * (-g[i] - ctz[i] - atv[i]);
}

__global__ void k_dual_eq_residual(int64_t n, const double* __restrict__ g, const double* __restrict__ dvec,
                                   const double* __restrict__ dx, const double* __restrict__ hc,
                                   const double* __restrict__ atv, const double* __restrict__ E,
                                   double* __restrict__ rho, double* __restrict__ erho) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const double r = -g[i] - (dvec[i] * dx[i] + hc[i]) - atv[i];
    rho[i] = r;
    erho[i] = E[i] * r;
  }
}

// dx += E o (rho - ctz - atv) over n entries, nu += nup over p entries (one grid over max(n, p))
__global__ void k_dual_eq_correct(int64_t n, int64_t p, const double* __restrict__ E, const double* __restrict__ rho,
                                  const double* __restrict__ ctz, const double* __restrict__ atv,
                                  double* __restrict__ dx, const double* __restrict__ nup, double* __restrict__ nu) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dx[i] = dx[i] + E[i] * (rho[i] - ctz[i] - atv[i]);
  if (i < p) nu[i] = nu[i] + nup[i];
}

// ---- the factored QP with equality rows (IPM_SOLVE_CHOLESKY_DUAL_QP_EQ): y = [z; nu] over M = [C; Pf; A]
// the equality block of M dx: adx = tail (= A dx, for rho_p), then tail = nu -- the stacked vector becomes
// [Mc dx; nu], which the weights [W; 1_p] turn into the one transposed product Mc^T (W o Mc dx) + A^T nu
__global__ void k_dual_qe_tail(int64_t p, double* __restrict__ tail, const double* __restrict__ nu,
                               double* __restrict__ adx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < p) {
    adx[i] = tail[i];
    tail[i] = nu[i];
  }
}

// nu += nup (p entries): the equality block of one refinement correction
__global__ void k_dual_qe_nu(int64_t p, const double* __restrict__ nup, double* __restrict__ nu) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < p) nu[i] = nu[i] + nup[i];
}

// ---- the dual-form PHASE-1 step (IPM_SOLVE_CHOLESKY_DUAL_PHASE1): the bordered system
// [[Hxx, h], [h^T, hss]] (dx, ds) = (-g_x, -g_s) with Hxx^-1 applied through S.  Scalars stay on the
// device in sc[]: every reduction is a fixed-order sum (per-thread strided partials, wave shuffles,
// then the waves in order), no atomics: two calls give the same bits.
constexpr int PH1_T = 1024;   // threads of the one-workgroup stages

// ru = E o (-g_x), ry = E o h: the two right-hand sides before C
__global__ void k_dual_ph1_rhs(int64_t n, const double* __restrict__ E, const double* __restrict__ g,
                               const double* __restrict__ h, double* __restrict__ ru, double* __restrict__ ry) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    ru[i] = E[i] * (-g[i]);
    ry[i] = E[i] * h[i];
  }
}

// u = E o (-g_x - C^T z_u) (into dx[0:n]), y = E o (h - C^T z_y): the two solutions of Hxx . = [-g_x | h]
__global__ void k_dual_ph1_uy(int64_t n, const double* __restrict__ E, const double* __restrict__ g,
                              const double* __restrict__ h, const double* __restrict__ ctzu,
                              const double* __restrict__ ctzy, double* __restrict__ u, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    u[i] = E[i] * (-g[i] - ctzu[i]);
    y[i] = E[i] * (h[i] - ctzy[i]);
  }
}

// sigma = hss - h.y, the Schur complement of Hxx in H~, in its form WITHOUT cancellation: H~ is a sum of
// squares over the slack rows, and (-y, 1) minimizes its quadratic form over (v, 1), so
//   sigma = sum_C w (1 + C y)^2 + sum inv_lb^2 (1 - y)^2 + sum inv_ub^2 (1 + y)^2 + add (y.y + 1)
// (the error of y enters squared; hss - h.y loses sigma / hss digits: 4.7e-9 on the test grid).
// Then ds = (-g_s - h.u) / sigma and dx = u - y ds (u arrives in dx[0:n]).  One workgroup.
// sc[0] = sigma, sc[1] = hss (+ add); *bad = 1 unless sigma is finite and positive.
__global__ __launch_bounds__(PH1_T) void k_dual_ph1_combine(int64_t n, int64_t m, const double* __restrict__ h,
                                                            const double* __restrict__ y,
                                                            const double* __restrict__ w,
                                                            const double* __restrict__ cy,
                                                            const double* __restrict__ ilb,
                                                            const double* __restrict__ iub,
                                                            const double* __restrict__ hss, double add,
                                                            const double* __restrict__ g, double* __restrict__ dx,
                                                            double* __restrict__ sc, int* __restrict__ bad) {
  __shared__ double red[16];
  double sg = 0.0, hu = 0.0;
  for (int64_t i = threadIdx.x; i < m; i += PH1_T) {
    const double a = 1.0 + cy[i];
    sg += w[i] * (a * a);
  }
  for (int64_t i = threadIdx.x; i < n; i += PH1_T) {
    const double yi = y[i];
    double v = add * (yi * yi);
    if (ilb) {
      const double a = 1.0 - yi, b = ilb[i];
      v += (b * b) * (a * a);
    }
    if (iub) {
      const double a = 1.0 + yi, b = iub[i];
      v += (b * b) * (a * a);
    }
    sg += v;
    hu = fma(h[i], dx[i], hu);
  }
  sg = block_sum(sg, red);
  hu = block_sum(hu, red);
  const double sigma = sg + add;
  const double ds = (-g[n] - hu) / sigma;
  for (int64_t i = threadIdx.x; i < n; i += PH1_T) dx[i] = dx[i] - y[i] * ds;
  if (threadIdx.x == 0) {
    dx[n] = ds;
    sc[0] = sigma;
    sc[1] = hss[0] + add;
    *bad = (isfinite(sigma) && sigma > 0.0) ? 0 : 1;
  }
}

// rho_x = -g_x - (D o dx + hc) - h ds with hc = C^T (w o (C dx)); erho = E o rho_x (the next solve's
// right-hand side before C); part[block] = the block's share of h.dx (for rho_s)
__global__ __launch_bounds__(256) void k_dual_ph1_residual(int64_t n, const double* __restrict__ g,
                                                           const double* __restrict__ dvec,
                                                           const double* __restrict__ dx,
                                                           const double* __restrict__ hc,
                                                           const double* __restrict__ h,
                                                           const double* __restrict__ E, double* __restrict__ rho,
                                                           double* __restrict__ erho, double* __restrict__ part) {
  __shared__ double red[16];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double ds = dx[n];
  double hd = 0.0;
  if (i < n) {
    const double r = -g[i] - (dvec[i] * dx[i] + hc[i]) - h[i] * ds;
    rho[i] = r;
    erho[i] = E[i] * r;
    hd = h[i] * dx[i];
  }
  hd = block_sum(hd, red);
  if (threadIdx.x == 0) part[blockIdx.x] = hd;
}

// du = E o (rho_x - C^T z'), rho_s = -g_s - h.dx - hss ds, dds = (rho_s - h.du) / sigma;
// dx += du - y dds, ds += dds.  One workgroup; h.dx from the residual launch's partials in block order.
__global__ __launch_bounds__(PH1_T) void k_dual_ph1_correct(int64_t n, int64_t nblk, const double* __restrict__ E,
                                                            const double* __restrict__ rho,
                                                            const double* __restrict__ ctz,
                                                            const double* __restrict__ h,
                                                            const double* __restrict__ y,
                                                            const double* __restrict__ g,
                                                            const double* __restrict__ sc,
                                                            const double* __restrict__ part, double* __restrict__ dx) {
  __shared__ double red[16];
  double hdx = 0.0, hdu = 0.0;
  for (int64_t b = threadIdx.x; b < nblk; b += PH1_T) hdx += part[b];
  for (int64_t i = threadIdx.x; i < n; i += PH1_T) hdu = fma(h[i], E[i] * (rho[i] - ctz[i]), hdu);
  hdx = block_sum(hdx, red);
  hdu = block_sum(hdu, red);
  const double ds = dx[n];
  const double rs = -g[n] - hdx - sc[1] * ds;
  const double dds = (rs - hdu) / sc[0];
  for (int64_t i = threadIdx.x; i < n; i += PH1_T) dx[i] = dx[i] + (E[i] * (rho[i] - ctz[i]) - y[i] * dds);
  __syncthreads();   // every thread has read ds = dx[n]
  if (threadIdx.x == 0) dx[n] = ds + dds;
}

// ---------------------------------------------------------------- launchers
// IPM_SOLVE_CHOLESKY_DUAL
// out = E * (-g - ctz): the last combination of the dual-form step, dx = E o (-g - C^T z)
void dual_combine(hipStream_t st, int64_t n, const double* E, const double* g, const double* ctz, double* out) {
  if (n > 0) hipLaunchKernelGGL(k_dual_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, g, ctz, out);
}

// rho = -g - (dvec o dx + hc): the primal residual of H dx = -g with hc = C^T (w o (C dx))
void dual_residual(hipStream_t st, int64_t n, const double* g, const double* dvec, const double* dx, const double* hc,
                   double* rho) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_residual, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, g, dvec, dx, hc, rho);
}

// dx += E o (rho - ctz): one refinement correction added in place
void dual_correct(hipStream_t st, int64_t n, const double* E, const double* rho, const double* ctz, double* dx) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_correct, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, rho, ctz, dx);
}

// IPM_SOLVE_CHOLESKY_DUAL_QP
void dual_qp_diag(hipStream_t st, int64_t n, const double* dvec, const double* pdiag, double t, double* D, double* E) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_qp_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, dvec, pdiag, t, D, E);
}

// IPM_SOLVE_CHOLESKY_DUAL_EQ
// r[i] -= -axb[i] - adx[i] (p entries; adx may be null): the equality block of the right-hand side
void dual_eq_rhs(hipStream_t st, int64_t p, const double* axb, const double* adx, double* r) {
  if (p > 0) hipLaunchKernelGGL(k_dual_eq_rhs, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, st, p, axb, adx, r);
}

// out = E o (-g - ctz - atv): dx from C^T z and A^T nu
void dual_eq_combine(hipStream_t st, int64_t n, const double* E, const double* g, const double* ctz, const double* atv,
                     double* out) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_eq_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, g, ctz, atv, out);
}

// rho = -g - (dvec o dx + hc) - atv, erho = E o rho: the first block row's residual of the KKT system
void dual_eq_residual(hipStream_t st, int64_t n, const double* g, const double* dvec, const double* dx,
                      const double* hc, const double* atv, const double* E, double* rho, double* erho) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_eq_residual, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, g, dvec, dx, hc, atv,
                       E, rho, erho);
}

void dual_eq_correct(hipStream_t st, int64_t n, int64_t p, const double* E, const double* rho, const double* ctz,
                     const double* atv, double* dx, const double* nup, double* nu) {
  const int64_t len = std::max(n, p);
  if (len > 0)
    hipLaunchKernelGGL(k_dual_eq_correct, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, n, p, E, rho, ctz, atv,
                       dx, nup, nu);
}

// IPM_SOLVE_CHOLESKY_DUAL_QP_EQ
void dual_qe_tail(hipStream_t st, int64_t p, double* tail, const double* nu, double* adx) {
  if (p > 0) hipLaunchKernelGGL(k_dual_qe_tail, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, st, p, tail, nu, adx);
}

void dual_qe_nu(hipStream_t st, int64_t p, const double* nup, double* nu) {
  if (p > 0) hipLaunchKernelGGL(k_dual_qe_nu, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, st, p, nup, nu);
}

// IPM_SOLVE_CHOLESKY_DUAL_PHASE1: g and dx have n + 1 entries (g[n] = g_s, dx[n] = ds)
void dual_ph1_rhs(hipStream_t st, int64_t n, const double* E, const double* g, const double* h, double* ru,
                  double* ry) {
  if (n > 0) hipLaunchKernelGGL(k_dual_ph1_rhs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, g, h, ru, ry);
}

void dual_ph1_uy(hipStream_t st, int64_t n, const double* E, const double* g, const double* h, const double* ctzu,
                 const double* ctzy, double* u, double* y) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_ph1_uy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, E, g, h, ctzu, ctzy, u, y);
}

// cy = C y; ilb / iub: the inverse bound slacks, either may be null
void dual_ph1_combine(hipStream_t st, int64_t n, int64_t m, const double* h, const double* y, const double* w,
                      const double* cy, const double* ilb, const double* iub, const double* hss, double add,
                      const double* g, double* dx, double* sc, int* bad) {
  hipLaunchKernelGGL(k_dual_ph1_combine, dim3(1), dim3(PH1_T), 0, st, n, m, h, y, w, cy, ilb, iub, hss, add, g, dx, sc,
                     bad);
}

// part: dual_ph1_blocks(n) entries
void dual_ph1_residual(hipStream_t st, int64_t n, const double* g, const double* dvec, const double* dx,
                       const double* hc, const double* h, const double* E, double* rho, double* erho, double* part) {
  if (n > 0)
    hipLaunchKernelGGL(k_dual_ph1_residual, dim3((unsigned)dual_ph1_blocks(n)), dim3(256), 0, st, n, g, dvec, dx, hc, h,
                       E, rho, erho, part);
}

void dual_ph1_correct(hipStream_t st, int64_t n, const double* E, const double* rho, const double* ctz, const double* h,
                      const double* y, const double* g, const double* sc, const double* part, double* dx) {
  hipLaunchKernelGGL(k_dual_ph1_correct, dim3(1), dim3(PH1_T), 0, st, n, dual_ph1_blocks(n), E, rho, ctz, h, y, g, sc,
                     part, dx);
}

// ---------------------------------------------------------------- the shared core
// M = [C; A], the A rows only with IPM_SOLVE_CHOLESKY_DUAL_EQ (dm = m + p); M = [C; Pf] with
// IPM_SOLVE_CHOLESKY_DUAL_QP (dm = m + kf); M = [C; Pf; A] with IPM_SOLVE_CHOLESKY_DUAL_QP_EQ (dm = m + kf + p);
// otherwise M = C, dm = m.
// y = M x (dm entries)
void m_apply(ipm_problem* pr, const double* x, double* y) {
  const ipm_problem_desc& d = pr->d;
  if (pr->dualqe) {   // all three blocks in one launch
    gemv_n3(S(pr), pr->n, x, pr->m, d.C, d.ldc, y, pr->kf, d.Pf, d.ldpf, y + pr->m, pr->p, d.A, d.lda,
            y + pr->m + pr->kf);
    return;
  }
  if (pr->dualqp) {   // both blocks in one launch
    gemv_n2(S(pr), pr->n, x, pr->m, d.C, d.ldc, y, pr->kf, d.Pf, d.ldpf, y + pr->m);
    return;
  }
  gemv_n(S(pr), pr->m, pr->n, 1.0, d.C, d.ldc, x, 0.0, y);
  if (pr->dualeq) gemv_n(S(pr), pr->p, pr->n, 1.0, d.A, d.lda, x, 0.0, y + pr->m);
}

// M^T [zc; za]: out = C^T (wc o zc) (wc null: no weights) and, with equality rows, pr->ATdv = A^T za; both
// halves in gemv_t's two-stage form (fixed order, no atomics) on the problem's partial-sum scratch
// (the factored QP: one stacked vector zc and stacked weights wc of dm entries, one launch pair over [C; Pf])
void mt_apply(ipm_problem* pr, const double* zc, const double* wc, const double* za, double* out) {
  const ipm_problem_desc& d = pr->d;
  if (pr->dualqe) {   // one stacked vector and stacked weights over [C; Pf; A], A^T nu included: za is not used
    gemv_t3(S(pr), pr->m, pr->kf, pr->p, pr->n, 1.0, d.C, d.ldc, d.Pf, d.ldpf, d.A, d.lda, zc, wc, 0.0, out, pr->part,
            pr->part_elems);
    return;
  }
  if (pr->dualqp) {
    gemv_t2(S(pr), pr->m, pr->kf, pr->n, 1.0, d.C, d.ldc, d.Pf, d.ldpf, zc, wc, 0.0, out, pr->part, pr->part_elems);
    return;
  }
  gemv_t(S(pr), pr->m, pr->n, 1.0, d.C, d.ldc, zc, wc, 0.0, out, pr->part, pr->part_elems);
  if (pr->dualeq) gemv_t(S(pr), pr->p, pr->n, 1.0, d.A, d.lda, za, nullptr, 0.0, pr->ATdv, pr->part, pr->part_elems);
}
// ... of one stacked vector z (dm entries), C's half into pr->dctz
void mt_apply(ipm_problem* pr, const double* z) { mt_apply(pr, z, nullptr, z + pr->m, pr->dctz); }

// K = diag(diw) + M diag(E) M^T into pr->dS, between timing events 0 and 1.  w and dvec are the primal
// SYRK's own vectors (psd add included): the same H; E = 1 / dvec, diw = 1 / w (with equality rows
// [1 / w; 0]: the zero tail is written at create).  Phase 1 forms its border here too, where the primal
// phase 1 forms it: h = -C^T inv_C^2 + inv_lb^2 - inv_ub^2 (pr->hxs), hss = sum inv^2 (scal slot SC_SUMINV2)
// The factored QP (t: the barrier parameter): D = dvec + t Pdiag into pr->dD, the stacked weights [w; t 1_kf] in
// pr->w (the tail refilled when t changes), diw = 1 / that, M = [C; Pf]
void assemble(ipm_problem* pr, double add, double t = 0.0) {
  const ipm_problem_desc& d = pr->d;
  ipm_handle* h = pr->h;
  hipStream_t st = S(pr);
  const int64_t m = pr->m, n = pr->n;
  if (h->timing) { hipEventRecord(h->ev[0], st); h->kkt_pending = true; }
  hessian_vectors_lin(pr, pr->s0, add);
  pr->hess_pre = false;
  if (pr->dual1) {
    mt_apply(pr, pr->inv, pr->inv, nullptr, pr->ct);
    border_vec_sq(st, n, pr->ct, inv_lb(pr), inv_ub(pr), pr->hxs);
    ReduceBatch rb{};
    rb.ops[0] = ReduceOp{pr->inv, nullptr, pr->S, 1, 1, RED_SUMSQ, SC_SUMINV2};
    reduce(st, rb, 1, pr->scal);
  }
  if (pr->dualqe) {
    // the factored QP with equality rows: W+ = [w; t 1_kf; 1_p] (the tail refilled when t changes), diw =
    // [1 / W; 0_p] (the zero tail written at create), M = [C; Pf; A]
    const int64_t mc = m + pr->kf;
    if (t != pr->dq_t) {
      if (pr->kf > 0) fill(st, pr->w + m, pr->kf, t);
      fill(st, pr->w + mc, pr->p, 1.0);
      pr->dq_t = t;
    }
    dual_qp_diag(st, n, pr->dvec, d.Pdiag, t, pr->dD, pr->dE);
    inv_eps(st, mc, pr->w, 0.0, pr->diw);
    syrk_nt_lower3(st, m, pr->kf, pr->p, n, d.C, d.ldc, d.Pf, d.ldpf, d.A, d.lda, pr->dE, pr->diw, pr->dS, pr->dlds,
                   pr->dsw);
    if (h->timing) hipEventRecord(h->ev[1], st);
    return;
  }
  if (pr->dualqp) {
    if (t != pr->dq_t) {
      if (pr->kf > 0) fill(st, pr->w + m, pr->kf, t);
      pr->dq_t = t;
    }
    dual_qp_diag(st, n, pr->dvec, d.Pdiag, t, pr->dD, pr->dE);
    inv_eps(st, pr->dm, pr->w, 0.0, pr->diw);
    syrk_nt_lower2(st, m, pr->kf, n, d.C, d.ldc, d.Pf, d.ldpf, pr->dE, pr->diw, pr->dS, pr->dlds, pr->dsw);
    if (h->timing) hipEventRecord(h->ev[1], st);
    return;
  }
  inv_eps(st, n, pr->dvec, 0.0, pr->dE);
  inv_eps(st, m, pr->w, 0.0, pr->diw);
  syrk_nt_lower2(st, m, pr->dm - m, n, d.C, d.ldc, d.A, d.lda, pr->dE, pr->diw, pr->dS, pr->dlds, pr->dsw);
  if (h->timing) hipEventRecord(h->ev[1], st);
}

// pr->dz = K^-1 pr->dr: the right-hand side rides through the bordered Cholesky as row dm (timing events 2
// and 3), which leaves L^-1 r there; one backward solve gives the solution
void factor_solve(ipm_problem* pr) {
  ipm_handle* h = pr->h;
  hipStream_t st = S(pr);
  const int64_t dm = pr->dm;
  if (h->timing) { hipEventRecord(h->ev[2], st); h->potrf_pending = true; }
  BorderJob bj;
  bj.N = dm;
  bj.H = pr->dS;
  bj.ldh = pr->dlds;
  bj.g = pr->dr;
  bj.scale = 1.0;
  potrf_lower_fused(st, dm + 1, pr->dS, pr->dlds, pr->info, pr->pws, dm, &bj);
  if (h->timing) hipEventRecord(h->ev[3], st);
  trsv_lower_t(st, dm, pr->dS, pr->dlds, pr->dS + dm, pr->dlds, pr->dz, pr->ctl, pr->xinv, trsv_err(pr));
}

// b <- K^-1 b (dm entries) on the factor: both triangles
void solve_on_factor(ipm_problem* pr, double* b) {
  potrs_lower(S(pr), pr->dm, 1, pr->dS, pr->dlds, b, 1, pr->dtw, pr->ctl, pr->xinv, trsv_err(pr));
}

// the step on an assembled K: H = diag(dv) + M^T diag(pr->w) M, M and K as m_apply / assemble have them
void direction_on_k(ipm_problem* pr, const double* dv);

}  // namespace

void pfactor_combine(hipStream_t st, int64_t n, const double* pdiag, const double* x, const double* ftfx, double* out) {
  if (n > 0)
    hipLaunchKernelGGL(k_pfactor_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, pdiag, x, ftfx, out);
}

void dual_direction(ipm_problem* pr, double add) {
  // the dual form: H = diag(dvec) + C^T diag(w) C, so with E = 1 / dvec
  //   S = diag(1 / w) + C diag(E) C^T,  z = S^-1 C (E o -g),  dx = E o (-g - C^T z)
  assemble(pr, add);
  direction_on_k(pr, pr->dvec);
}

void dual_direction_qp(ipm_problem* pr, double add, double t) {
  // the dual form for P = diag(Pdiag) + Pf^T Pf: H = diag(D) + M^T diag(W) M with
  // D = dvec + t Pdiag, M = [C; Pf], W = [w; t 1_kf], so method 6's step with K = diag(1 / W) + M diag(E) M^T
  // of order m + kf in place of S: the same launches over the stacked operand
  assemble(pr, add, t);
  direction_on_k(pr, pr->dD);
}

namespace {
void direction_on_k(ipm_problem* pr, const double* dv) {
  hipStream_t st = S(pr);
  const int64_t n = pr->n;
  // border row r = C (E o -g); the bordered Cholesky leaves L^-1 r in row m, one backward solve gives z
  mul(st, n, pr->dE, pr->g, -1.0, pr->tmpn);
  m_apply(pr, pr->tmpn, pr->dr);
  factor_solve(pr);
  mt_apply(pr, pr->dz);
  dual_combine(st, n, pr->dE, pr->g, pr->dctz, pr->dx);
  for (int round = 0; round < pr->drefine; ++round) {
    // rho = -g - H dx with H applied as diag(dvec) + C^T diag(w) C, never formed
    m_apply(pr, pr->dx, pr->dz);
    mt_apply(pr, pr->dz, pr->w, nullptr, pr->dctz);
    dual_residual(st, n, pr->g, dv, pr->dx, pr->dctz, pr->drho);
    // dx += E o (rho - C^T z'),  z' = S^-1 C (E o rho): both triangles of the factor this time
    mul(st, n, pr->dE, pr->drho, 1.0, pr->tmpn);
    m_apply(pr, pr->tmpn, pr->dr);
    solve_on_factor(pr, pr->dr);
    mt_apply(pr, pr->dr);
    dual_correct(st, n, pr->dE, pr->drho, pr->dctz, pr->dx);
  }
}
}  // namespace

void dual_direction_phase1(ipm_problem* pr, double add) {
  // the dual form of the phase-1 step.  H~ = [[Hxx, h], [h^T, hss]] with
  // Hxx = diag(dvec) + C^T diag(w) C -- the matrix dual_direction inverts -- and the
  // variable s one bordering column:
  //   y = Hxx^-1 h,  u = Hxx^-1 (-g_x)      (one factorization of S, two right-hand sides)
  //   sigma = hss - h.y (formed as a sum of squares, without cancellation),
  //   ds = (-g_s - h.u) / sigma,  dx = u - y ds
  // w, dvec, h and hss are the vectors the primal phase 1 puts into H~ (psd add on dvec and hss)
  const ipm_problem_desc& d = pr->d;
  hipStream_t st = S(pr);
  const int64_t m = pr->m, n = pr->n;
  assemble(pr, add);
  // R = C (E o [-g_x | h]): column u rides through the bordered Cholesky, column y is solved on the factor
  // (both columns in one pass over C, and over C^T below: the helpers' one-vector products do not say that)
  dual_ph1_rhs(st, n, pr->dE, pr->g, pr->hxs, pr->tmpn, pr->d1ry);
  gemv_n_2v(st, m, n, d.C, d.ldc, pr->tmpn, pr->d1ry, pr->dr, pr->d1zy);
  factor_solve(pr);
  solve_on_factor(pr, pr->d1zy);
  gemv_t_2v(st, m, n, d.C, d.ldc, pr->dz, pr->d1zy, pr->dctz, pr->d1cty, pr->part, pr->part_elems);
  dual_ph1_uy(st, n, pr->dE, pr->g, pr->hxs, pr->dctz, pr->d1cty, pr->dx, pr->d1y);
  // sigma in its sum-of-squares form needs C y (one more pass over C per step; hss - h.y cancels)
  m_apply(pr, pr->d1y, pr->d1zy);
  dual_ph1_combine(st, n, m, pr->hxs, pr->d1y, pr->w, pr->d1zy, inv_lb(pr), inv_ub(pr), pr->scal + SC_SUMINV2, add,
                   pr->g, pr->dx, pr->d1sc, pr->info + RB_INFO_DUAL1);
  for (int round = 0; round < pr->drefine; ++round) {
    // the residual of the FULL bordered system, H~ applied through C and never formed:
    //   rho_x = -g_x - (D o dx + C^T (w o (C dx))) - h ds,  rho_s = -g_s - h.dx - hss ds
    m_apply(pr, pr->dx, pr->dz);
    mt_apply(pr, pr->dz, pr->w, nullptr, pr->dctz);
    dual_ph1_residual(st, n, pr->g, pr->dvec, pr->dx, pr->dctz, pr->hxs, pr->dE, pr->drho, pr->tmpn, pr->d1part);
    // du = E o (rho_x - C^T S^-1 C (E o rho_x)),  dds = (rho_s - h.du) / sigma;  dx += du - y dds, ds += dds
    m_apply(pr, pr->tmpn, pr->dr);
    solve_on_factor(pr, pr->dr);
    mt_apply(pr, pr->dr);
    dual_ph1_correct(st, n, pr->dE, pr->drho, pr->dctz, pr->hxs, pr->d1y, pr->g, pr->d1sc, pr->d1part, pr->dx);
  }
}

void dual_direction_eq(ipm_problem* pr, const double* v, double add) {
  // the dual form with equality rows.  H = diag(dvec) + C^T diag(w) C; with E = 1 / dvec,
  // z = w o (C dx) and M = [C; A], eliminating dx = E o (-g - C^T z - A^T nu) from
  //   H dx + A^T nu = -g,  A dx = -(A x - b)
  // leaves K [z; nu] = [C (E o -g); A (E o -g) + (A x - b)],  K = diag([1 / w; 0]) + M diag(E) M^T,
  // positive definite when A has full row rank.  The psd add goes on dvec only.  No n x n and no n x p array.
  const ipm_problem_desc& d = pr->d;
  hipStream_t st = S(pr);
  const int64_t m = pr->m, n = pr->n, p = pr->p;
  double *nu = pr->dz + m, *rp = pr->dr + m;   // the equality blocks of the solution and the right-hand side
  assemble(pr, add);
  // the stacked right-hand side rides through the bordered Cholesky as row m + p
  mul(st, n, pr->dE, pr->g, -1.0, pr->tmpn);
  m_apply(pr, pr->tmpn, pr->dr);
  dual_eq_rhs(st, p, pr->Axb, nullptr, rp);
  factor_solve(pr);
  mt_apply(pr, pr->dz);
  dual_eq_combine(st, n, pr->dE, pr->g, pr->dctz, pr->ATdv, pr->dx);
  for (int round = 0; round < pr->drefine; ++round) {
    // the residual of the FULL KKT system, H applied through C and never formed:
    //   rho_x = -g - (D o dx + C^T (w o (C dx))) - A^T nu,  rho_p = -(A x - b) - A dx
    // (C dx and A dx in launches of their own: the first feeds the weighted C^T product, the second rho_p)
    gemv_n(st, m, n, 1.0, d.C, d.ldc, pr->dx, 0.0, pr->dtw);
    mt_apply(pr, pr->dtw, pr->w, nu, pr->dctz);
    dual_eq_residual(st, n, pr->g, pr->dvec, pr->dx, pr->dctz, pr->ATdv, pr->dE, pr->drho, pr->tmpn);
    gemv_n(st, p, n, 1.0, d.A, d.lda, pr->dx, 0.0, pr->Adx);
    // [z'; nu'] = K^-1 [C (E o rho_x); A (E o rho_x) - rho_p] on the factor; dx += E o (rho_x - M^T [z'; nu']),
    // nu += nu'
    m_apply(pr, pr->tmpn, pr->dr);
    dual_eq_rhs(st, p, pr->Axb, pr->Adx, rp);
    solve_on_factor(pr, pr->dr);
    mt_apply(pr, pr->dr);
    dual_eq_correct(st, n, p, pr->dE, pr->drho, pr->dctz, pr->ATdv, pr->dx, rp, nu);
  }
  lincomb(st, p, 1.0, nu, -1.0, v, pr->dv);   // dv = nu - v
}

void dual_direction_qp_eq(ipm_problem* pr, const double* v, double add, double t) {
  // the factored QP with equality rows.  H = diag(D) + Mc^T diag(W) Mc with Mc = [C; Pf],
  // W = [w; t 1_kf], D = dvec + t Pdiag; with E = 1 / D, z = W o (Mc dx), M = [C; Pf; A] and y = [z; nu],
  // eliminating dx = E o (-g - M^T y) from  H dx + A^T nu = -g,  A dx = -(A x - b)  leaves
  //   K y = [Mc (E o -g); A (E o -g) + (A x - b)],  K = diag([1 / W; 0_p]) + M diag(E) M^T   (order m + kf + p),
  // positive definite when A has full row rank.  The psd add goes on D only.  No n x n and no n x p array.
  // The x-part's elementwise kernels are method 6's: M^T y is ONE transposed product over the three blocks.
  hipStream_t st = S(pr);
  const int64_t n = pr->n, p = pr->p, mc = pr->m + pr->kf;
  double *nu = pr->dz + mc, *rp = pr->dr + mc;   // the equality blocks of the solution and the right-hand side
  assemble(pr, add, t);
  // the stacked right-hand side rides through the bordered Cholesky as row m + kf + p
  mul(st, n, pr->dE, pr->g, -1.0, pr->tmpn);
  m_apply(pr, pr->tmpn, pr->dr);
  dual_eq_rhs(st, p, pr->Axb, nullptr, rp);
  factor_solve(pr);
  mt_apply(pr, pr->dz);
  dual_combine(st, n, pr->dE, pr->g, pr->dctz, pr->dx);
  for (int round = 0; round < pr->drefine; ++round) {
    // the residual of the FULL KKT system, H applied through Mc and never formed:
    //   rho_x = -g - (D o dx + M^T ([W; 1_p] o [Mc dx; nu])),  rho_p = -(A x - b) - A dx
    // (M dx in one launch; its equality block goes to Adx and is replaced by nu)
    m_apply(pr, pr->dx, pr->dtw);
    dual_qe_tail(st, p, pr->dtw + mc, nu, pr->Adx);
    mt_apply(pr, pr->dtw, pr->w, nullptr, pr->dctz);
    dual_residual(st, n, pr->g, pr->dD, pr->dx, pr->dctz, pr->drho);
    // y' = K^-1 [Mc (E o rho_x); A (E o rho_x) - rho_p] on the factor; dx += E o (rho_x - M^T y'), nu += nu'
    mul(st, n, pr->dE, pr->drho, 1.0, pr->tmpn);
    m_apply(pr, pr->tmpn, pr->dr);
    dual_eq_rhs(st, p, pr->Axb, pr->Adx, rp);
    solve_on_factor(pr, pr->dr);
    mt_apply(pr, pr->dr);
    dual_correct(st, n, pr->dE, pr->drho, pr->dctz, pr->dx);
    dual_qe_nu(st, p, rp, nu);
  }
  lincomb(st, p, 1.0, nu, -1.0, v, pr->dv);   // dv = nu - v
}

}  // namespace ipm
