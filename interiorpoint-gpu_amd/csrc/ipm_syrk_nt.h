// Weighted SYRK over the CONTIGUOUS index of a row-major operand (ipm_syrk_nt.hip): the assembly of the
// dual-form Newton steps (ipm_dual.hip).
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
// ... and on the (m0 + m1 + m2) x k matrix of three row blocks X0, X1, X2 (each with its own leading dimension):
// the plan of syrk_nt_plan(m0 + m1 + m2, k), bit for bit syrk_nt_lower on the stacked matrix; a 64-row block may
// straddle either seam or both.  16-byte loads only when all three operands qualify.  An empty block's pointer
// is never read: m2 == 0 is syrk_nt_lower2 on (X0, X1), and so on down to syrk_nt_lower.
void syrk_nt_lower3(hipStream_t s, int64_t m0, int64_t m1, int64_t m2, int64_t k, const double* X0, int64_t ldx0,
                    const double* X1, int64_t ldx1, const double* X2, int64_t ldx2, const double* w,
                    const double* dvec, double* H, int64_t ldh, double* ws);

}  // namespace ipm
