// Conjugate-gradient Newton step (ipm_cg.hip): a symmetric matrix-vector product on the
// lower-triangle layout assemble_hessian writes, and scipy.sparse.linalg.cg's loop as a fixed
// launch sequence (NewtonSolver.py:365-400).  No workgroup waits on another: every stage is its
// own launch, cross-workgroup sums go through per-tile partials that a later launch adds in a
// fixed order, so results are bitwise repeatable.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace ipm {

constexpr int SYMV_T = 128;   // tile edge of the SYMV (rows and columns)

inline int64_t symv_blocks(int64_t n) { return (n + SYMV_T - 1) / SYMV_T; }
// per-tile partials: for each of the nb output blocks one 128-vector from every block of its
// block row and block column (nb slots)
inline int64_t symv_ws_doubles(int64_t n) {
  const int64_t nb = symv_blocks(n);
  return std::max<int64_t>(nb * nb * SYMV_T, 1);
}
// y = alpha * H x + beta * y; H symmetric, only its lower triangle (column-major, ldh >= n) is
// read; beta == 0 never reads y.  ws: symv_ws_doubles(n)
void symv_lower(hipStream_t s, int64_t n, double alpha, const double* H, int64_t ldh, const double* x, double beta,
                double* y, double* ws);

// CG workspace: scalars and control words, r, p, q, the p.q partials, the SYMV partials, then the
// preconditioner's diagonal minv (nb * 128, last so that no other offset moves)
inline int64_t cg_ws_doubles(int64_t n) {
  const int64_t nb = symv_blocks(n);
  return 16 + 3 * nb * SYMV_T + nb + 8 + symv_ws_doubles(n) + nb * SYMV_T;
}
// the minv region of a cg_ws_doubles(n) workspace
double* cg_ws_minv(int64_t n, double* ws);
// minv[i] = 1 / H[i + i ldh] for i < n, 0 up to nb * 128 (the Jacobi preconditioner).  Nothing is
// special-cased: a zero, negative or NaN diagonal entry propagates as the arithmetic gives it, the
// solve then ends with info = maxiter after the usual maxiter rounds of launches.
void cg_minv(hipStream_t s, int64_t n, const double* H, int64_t ldh, double* minv);
// solve H x = bsign * b with scipy.sparse.linalg.cg's loop (rtol, atol = 0): x holds x0 on entry.
// minv == nullptr: no preconditioner.  Otherwise M = diag(minv) (device, n entries read), scipy's
// loop with M: the convergence test on r, z = M r, rho = r.z, p = (rho / rho_prev) p + z.
// res (device, 2 ints): iterations done, info (0 converged / maxiter).
// A fixed sequence of 3 launches per iteration for maxiter iterations; once the device `done`
// word is set every later launch returns at once and x is not touched again.
void cg_solve(hipStream_t s, int64_t n, const double* H, int64_t ldh, const double* b, double bsign, double* x,
              int32_t maxiter, double rtol, double* ws, int* res, const double* minv = nullptr);
// NewtonSolver.py:379-383 on the device: dc = xc.g; x0 = (-dc * xc) / (xc.(H xc)) if dc < 0 (the
// SYMV runs only then) else 0
void cg_warm_start(hipStream_t s, int64_t n, const double* H, int64_t ldh, const double* xc, const double* g,
                   double* x0, double* ws);

}  // namespace ipm
