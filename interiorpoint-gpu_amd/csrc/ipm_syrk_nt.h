// Weighted SYRK over the CONTIGUOUS index of a row-major operand (ipm_syrk_nt.hip), and the small
// vector kernel of the dual-form Newton step (IPM_SOLVE_CHOLESKY_DUAL) that uses it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace ipm {

constexpr int SYRK_NT_TILE = 64;   // output tile (rows and columns of H per workgroup)
constexpr int SYRK_NT_BK = 32;     // k columns per LDS stage; K chunks are multiples of it

// launch plan: T x T lower-triangle tiles; with fewer tiles than compute units the k range is cut
// into ks chunks of `chunk` columns (a multiple of SYRK_NT_BK; the last one may be ragged, none is
// empty), one workgroup each, whose partial tiles a second launch adds in chunk order
struct SyrkNtPlan {
  int64_t T = 0, ntiles = 0, ks = 1, chunk = 0;
};
inline SyrkNtPlan syrk_nt_plan(int64_t m, int64_t k) {
  SyrkNtPlan p;
  p.T = (m + SYRK_NT_TILE - 1) / SYRK_NT_TILE;
  p.ntiles = p.T * (p.T + 1) / 2;
  const int64_t kk = std::max<int64_t>(k, 1);
  p.chunk = (kk + SYRK_NT_BK - 1) / SYRK_NT_BK * SYRK_NT_BK;
  if (p.ntiles < 256 && k > 512) {
    // about two workgroups per compute unit, no chunk shorter than 256 columns
    const int64_t want = std::min<int64_t>((512 + p.ntiles - 1) / p.ntiles, (k + 255) / 256);
    p.chunk = ((k + want - 1) / want + SYRK_NT_BK - 1) / SYRK_NT_BK * SYRK_NT_BK;
    p.ks = (k + p.chunk - 1) / p.chunk;
  }
  return p;
}
// partial tiles of the K split (0 doubles when the plan does not split)
inline int64_t syrk_nt_ws_doubles(int64_t m, int64_t k) {
  if (m <= 0) return 0;
  const SyrkNtPlan p = syrk_nt_plan(m, k);
  return p.ks > 1 ? p.ntiles * p.ks * SYRK_NT_TILE * SYRK_NT_TILE : 0;
}
// lower triangle (column-major, ldh >= m) of H(i, j) = sum_kk X[i][kk] w[kk] X[j][kk] (+ dvec[i] on
// the diagonal); X row-major m x k (ldx >= k); w (k) and dvec (m) may be null (all ones / no diagonal
// term).  Overwrites: H is never read; the strict upper triangle and everything beyond row / column
// m stay untouched.  ws: syrk_nt_ws_doubles(m, k) doubles (null: no K split).  No atomics: bitwise
// repeatable.
void syrk_nt_lower(hipStream_t s, int64_t m, int64_t k, const double* X, int64_t ldx, const double* w,
                   const double* dvec, double* H, int64_t ldh, double* ws);
// the same product on the (m0 + m1) x k matrix whose first m0 rows are X0's (ldx0) and whose last m1 rows are
// X1's (ldx1), neither copied: plan, K split, workspace (syrk_nt_ws_doubles(m0 + m1, k)) and fold order are
// those of syrk_nt_lower on the stacked matrix, so the result equals it bit for bit.  16-byte loads only when
// both operands qualify.  m1 == 0: syrk_nt_lower on X0.
void syrk_nt_lower2(hipStream_t s, int64_t m0, int64_t m1, int64_t k, const double* X0, int64_t ldx0,
                    const double* X1, int64_t ldx1, const double* w, const double* dvec, double* H, int64_t ldh,
                    double* ws);
// ---- IPM_SOLVE_CHOLESKY_DUAL_EQ: the dual form with equality rows, K [z; nu] = r over M = [C; A]
// r[i] -= -axb[i] - adx[i] (p entries; adx may be null): the equality block of the right-hand side,
// A (E o rho_x) - rho_p with rho_p = -(A x - b) - A dx
void dual_eq_rhs(hipStream_t s, int64_t p, const double* axb, const double* adx, double* r);
// out = E o (-g - ctz - atv): dx from C^T z and A^T nu
void dual_eq_combine(hipStream_t s, int64_t n, const double* E, const double* g, const double* ctz, const double* atv,
                     double* out);
// rho = -g - (dvec o dx + hc) - atv, erho = E o rho: the first block row's residual of the KKT system
void dual_eq_residual(hipStream_t s, int64_t n, const double* g, const double* dvec, const double* dx,
                      const double* hc, const double* atv, const double* E, double* rho, double* erho);
// dx += E o (rho - ctz - atv) (n entries), nu += nup (p entries)
void dual_eq_correct(hipStream_t s, int64_t n, int64_t p, const double* E, const double* rho, const double* ctz,
                     const double* atv, double* dx, const double* nup, double* nu);
// out = E * (-g - ctz): the last combination of the dual-form step, dx = E o (-g - C^T z)
void dual_combine(hipStream_t s, int64_t n, const double* E, const double* g, const double* ctz, double* out);
// rho = -g - (dvec o dx + hc): the primal residual of H dx = -g with hc = C^T (w o (C dx))
void dual_residual(hipStream_t s, int64_t n, const double* g, const double* dvec, const double* dx, const double* hc,
                   double* rho);
// dx += E o (rho - ctz): one refinement correction added in place
void dual_correct(hipStream_t s, int64_t n, const double* E, const double* rho, const double* ctz, double* dx);

// ---- IPM_SOLVE_CHOLESKY_DUAL_PHASE1: the bordered system [[Hxx, h], [h^T, hss]] (dx, ds) = (-g_x, -g_s),
// Hxx = diag(D) + C^T diag(w) C applied / inverted as in the phase-2 dual step.  g and dx have n + 1
// entries (g[n] = g_s, dx[n] = ds).  All reductions in a fixed order, no atomics, scalars on the device.
// ru = E o (-g_x), ry = E o h
void dual_ph1_rhs(hipStream_t s, int64_t n, const double* E, const double* g, const double* h, double* ru, double* ry);
// u = E o (-g_x - ctzu), y = E o (h - ctzy)
void dual_ph1_uy(hipStream_t s, int64_t n, const double* E, const double* g, const double* h, const double* ctzu,
                 const double* ctzy, double* u, double* y);
// dx[0:n] holds u on entry.  sc[0] = sigma = sum w (1 + cy)^2 + sum ilb^2 (1 - y)^2 + sum iub^2 (1 + y)^2 +
// add (y.y + 1) with cy = C y (the cancellation-free form of hss - h.y; ilb / iub: the inverse bound slacks,
// either may be null), sc[1] = hss[0] + add; dx[n] = ds = (-g_s - h.u) / sigma, dx[0:n] = u - y ds;
// *bad = 1 unless sigma is finite and positive
void dual_ph1_combine(hipStream_t s, int64_t n, int64_t m, const double* h, const double* y, const double* w,
                      const double* cy, const double* ilb, const double* iub, const double* hss, double add,
                      const double* g, double* dx, double* sc, int* bad);
// rho = -g_x - (dvec o dx + hc) - h ds, erho = E o rho, part[b] = block b's share of h.dx
// (dual_ph1_blocks(n) entries)
inline int64_t dual_ph1_blocks(int64_t n) { return (n + 255) / 256; }
void dual_ph1_residual(hipStream_t s, int64_t n, const double* g, const double* dvec, const double* dx,
                       const double* hc, const double* h, const double* E, double* rho, double* erho, double* part);
// du = E o (rho - ctz), dds = ((-g_s - sum part - sc[1] ds) - h.du) / sc[0]; dx[0:n] += du - y dds, dx[n] += dds
void dual_ph1_correct(hipStream_t s, int64_t n, const double* E, const double* rho, const double* ctz, const double* h,
                      const double* y, const double* g, const double* sc, const double* part, double* dx);

}  // namespace ipm
